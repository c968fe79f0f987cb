/*
 * rmgr/ssim-hip.h -- the C ABI of the MI355X (gfx950) SSIM engine.
 *
 * This is the drop-in boundary: plain C, pointers and sizes only, no HIP / torch / C++ types.
 * <rmgr/ssim.h>'s entry points are thin C++98 wrappers over it (ssim_amd/csrc/ssim_dropin.cpp),
 * and any other host (ctypes, cgo, JNI ...) binds these symbols directly -- see INTEGRATION.md.
 *
 * Each function names the reference interface it stands in for (file:line in romigrou/ssim):
 *
 *   rmgr_ssim_hip_compute_ssim_host    rmgr::ssim::compute_ssim           src/ssim.cpp:933-1106
 *   rmgr_ssim_hip_compute_ssim_device  same, images/map already in HBM    src/ssim.cpp:933-1106
 *   rmgr_ssim_hip_compute_ssim_batch_host  a caller's loop over host pairs  sample/rmgr-ssim-sample.cpp:84-95
 *   rmgr_ssim_hip_compute_ssim_batch_host_devices  the same over several GPUs   src/ssim.cpp:1048-1088 (thread-pool dispatch)
 *   rmgr_ssim_hip_enqueue_batch        the caller-side loop over pairs    src/ssim-cli.cpp:197-210
 *                                      + per-thread fp64 partials         src/ssim.cpp:902-926
 *   rmgr_ssim_hip_enqueue_rows / _reduce_cells   one image's tile jobs split over workers   src/ssim.cpp:1048-1100
 *   rmgr_ssim_hip_finalize             the final mean                     src/ssim.cpp:1090-1103
 *   rmgr_ssim_hip_compute_ssim_channels_host   the per-channel caller loop       src/ssim-cli.cpp:197-210, sample/rmgr-ssim-sample.cpp:82-101
 *   rmgr_ssim_hip_compute_ssim_luminance_host  RGB -> BT.601 Y, then SSIM        src/ssim-cli.cpp:145-195
 *   rmgr_ssim_hip_luminance_device             the conversion loop alone          src/ssim-cli.cpp:158-186
 *   rmgr_ssim_hip_set_mode             select_impl() / RMGR_SSIM_USE_DOUBLE   src/ssim.cpp:808-896, src/ssim_internal.h:26-37
 *   rmgr_ssim_hip_compute_msssim_device / _host   multi-scale SSIM: no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_ssim16, rmgr_ssim_hip_compute_ssim16_device / _host   SSIM of 9- to 16-bit samples: no reference
 *                                      counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_msssimf, rmgr_ssim_hip_compute_msssimf_device / _host, rmgr_ssim_hip_enqueue_msssimf_grad   multi-scale SSIM
 *       of float32 images and its gradient: no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_ssimf, rmgr_ssim_hip_compute_ssimf_device / _host, rmgr_ssim_hip_enqueue_ssimf_grad   SSIM of float32
 *                                      samples and its gradient: no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_ssimh, rmgr_ssim_hip_compute_ssimh_device / _host, rmgr_ssim_hip_enqueue_ssimh_grad   SSIM of float16 /
 *                                      bfloat16 samples and its gradient: no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_msssimh, rmgr_ssim_hip_compute_msssimh_device / _host, rmgr_ssim_hip_enqueue_msssimh_grad   multi-scale SSIM
 *       of float16 / bfloat16 images and its gradient: no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_ssimf_map_grad, rmgr_ssim_hip_enqueue_ssimh_map_grad   gradient of the SSIM MAP for a per-pixel upstream
 *                                      gradient: no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_ssimh_win, rmgr_ssim_hip_compute_ssimh_win_device / _host, rmgr_ssim_hip_enqueue_ssimh_win_grad,
 *   rmgr_ssim_hip_enqueue_ssimh_win_map_grad   the float16 / bfloat16 entries under a caller-chosen window (size, sigma, box): no
 *                                      reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_msssimf_win, rmgr_ssim_hip_compute_msssimf_win_device / _host, rmgr_ssim_hip_enqueue_msssimf_win_grad and
 *   the four msssimh_win counterparts          the multi-scale float32 and float16 / bfloat16 entries under a caller-chosen window:
 *                                      no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_ssim3f, rmgr_ssim_hip_compute_ssim3f_device / _host, rmgr_ssim_hip_enqueue_ssim3f_grad   SSIM of float32
 *                                      VOLUMES (three-dimensional window) and its gradient: no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_ssim3f_map_grad      gradient of the 3-D SSIM MAP for a per-voxel upstream gradient: no reference
 *                                      counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_ssim3h, rmgr_ssim_hip_compute_ssim3h_device / _host, rmgr_ssim_hip_enqueue_ssim3h_grad,
 *   rmgr_ssim_hip_enqueue_ssim3h_map_grad      the same three for float16 / bfloat16 VOLUMES: no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_ssim3f_win, rmgr_ssim_hip_compute_ssim3f_win_device / _host, rmgr_ssim_hip_enqueue_ssim3f_win_grad,
 *   rmgr_ssim_hip_enqueue_ssim3f_win_map_grad  the float32 VOLUME entries under a caller-chosen window (size, sigma, box): no reference
 *                                      counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_ssim3h_win, rmgr_ssim_hip_compute_ssim3h_win_device / _host, rmgr_ssim_hip_enqueue_ssim3h_win_grad,
 *   rmgr_ssim_hip_enqueue_ssim3h_win_map_grad  the float16 / bfloat16 VOLUME entries under a caller-chosen window: no reference
 *                                      counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_msssim3f, rmgr_ssim_hip_compute_msssim3f_device / _host, rmgr_ssim_hip_enqueue_msssim3f_grad   multi-scale
 *                                      SSIM of float32 VOLUMES and its gradient: no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_msssim3h, rmgr_ssim_hip_compute_msssim3h_device / _host, rmgr_ssim_hip_enqueue_msssim3h_grad   multi-scale
 *                                      SSIM of float16 / bfloat16 VOLUMES and its gradient: no reference counterpart (definition below)
 *   rmgr_ssim_hip_enqueue_msssim3f_win, rmgr_ssim_hip_compute_msssim3f_win_device / _host, rmgr_ssim_hip_enqueue_msssim3f_win_grad and
 *   the four msssim3h_win counterparts         the multi-scale float32 and float16 / bfloat16 VOLUME entries under a caller-chosen
 *                                      window: no reference counterpart (definition below)
 *
 * All functions return 0 or an errno value (EINVAL, ENOMEM, ECHILD = a HIP call failed,
 * ENODEV = no gfx950 device / extension not usable), exactly like the reference's API; the multi-GPU
 * exchange (rmgr_ssim_hip_comm_*) adds ENOSYS = no librccl and ETIMEDOUT = a peer rank did not arrive in time.
 */
#ifndef RMGR_SSIM_HIP_H
#define RMGR_SSIM_HIP_H

#include <rmgr/ssim.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Arithmetic of the blur + SSIM stage. */
#define RMGR_SSIM_HIP_MODE_EXACT   0  /* operation order of the reference's FMA path (src/ssim_fma.cpp:196-257,
                                         src/ssim_avx.cpp:342-352): bit-identical per-pixel results. Default. */
#define RMGR_SSIM_HIP_MODE_FAST    1  /* the three E[.] planes in the reference's exact operation order (bit-identical planes), the two
                                         mu planes by a separable 11+11 fp32 blur: not bit-identical, but inside the reference's
                                         documented single-precision tolerance RELATIVE TO ITS FMA PATH (global 1.5e-6, per pixel
                                         6.3e-4) on all five of the reference's test image sets, with >= 30 % / >= 60 % margin.  (On large flat
                                         areas every pixel's rounding error has the same sign and the GLOBAL value can differ more --
                                         DESIGN.md section 2; only modes 0 and 3 are guarantees) */
#define RMGR_SSIM_HIP_MODE_DOUBLE  2  /* RMGR_SSIM_USE_DOUBLE semantics: fp64 internals, true double kernel (tests/ssim_naive.h) */
#define RMGR_SSIM_HIP_MODE_UNFUSED 3  /* operation order of the reference's AVX/SSE/generic paths (mul and add rounded separately) */
#define RMGR_SSIM_HIP_MODE_SEPARABLE 4 /* every plane by the separable 11+11 fp32 blur (four planes, centred pixels): the fastest mode and
                                         closer to the exact value than the reference's own fp32 paths (<= 2e-4 per pixel), inside the
                                         reference's TEST tolerances against its double oracle (2e-6 / 1e-3) -- but not correlated with
                                         the reference's rounding, hence NOT guaranteed within 6.3e-4 of its FMA path per pixel */

/* Version of THIS header's interface (the rmgr_ssim_hip_* functions and structs), independent of the reference API's
 * 2.1.0 that rmgr_ssim_get_version() reports.  Bumped whenever a struct layout, a function signature or the meaning of a
 * constant changes; rmgr_ssim_hip_get_abi_version() returns the value the LIBRARY was built with, so a client can
 * refuse a mismatch at start-up.  History (INTEGRATION.md has the migration notes):
 *   3  round 3: MODE_FAST (1) became the hybrid, the all-separable arithmetic moved to MODE_SEPARABLE (4); Plan grew by two fields
 *   4  round 4: Plan carries structSize (first field) and the cell grid; rmgr_ssim_hip_comm_* calls are bounded by a deadline
 *      (ETIMEDOUT), comm_rank_count / comm_describe added; row-band entry points (enqueue_rows, reduce_cells) added
 *   5  round 5: MODE_FAST (1) and MODE_SEPARABLE (4) form their quotient as n * rcp(d): their values moved by <= 3 ulp (contracts unchanged); ctx == NULL calls
 *      run on a pool of default contexts and no longer serialise; Plan grew by balancedChunks / balancedChunkRows (harmless: structSize);
 *      the deadline of synchronize / destroy applies per queued all-reduce; get_default_pool, get_kernel_source_id added
 *   6  round 6: additions only -- probe_valu, get_profile_clock, tune / get_tuned / set_tuned / clear_tuned, trim / trim_default_pool / get_default_pool_memory / get_memory_info; the default contexts
 *      release staging above $RMGR_SSIM_HIP_POOL_RETAIN_MB when a call ends; a threadPool with a dispatch function IS called (one job per row band, ECHILD
 *      when it fails); Plan: balancedInterleave appended (harmless: structSize), tuning variants 7 and 100 + T; set_mode / get_mode(NULL) no longer wait for a lease */
#define RMGR_SSIM_HIP_ABI_VERSION 6
rmgr_int32_t rmgr_ssim_hip_get_abi_version(void) RMGR_NOEXCEPT;

/* sha256 (hex) of the kernel source this library's device code was compiled from ("unknown" when it was not built by the Makefile).
 * Measurements tied to one version of the kernels -- profiles/traffic.json -- record it, and bench.py quotes them only for that version. */
const char* rmgr_ssim_hip_get_kernel_source_id(void) RMGR_NOEXCEPT;

/* The default contexts of the ctx == NULL entry points (see rmgr_ssim_hip_compute_ssim_host): how many exist right now and how many
 * calls may be in flight at a time.  Either pointer may be NULL.  Creates nothing. */
rmgr_int32_t rmgr_ssim_hip_get_default_pool(rmgr_int32_t* contexts, rmgr_int32_t* limit) RMGR_NOEXCEPT;

/* Memory policy of the default contexts.  A context's staging -- device copies of the images and the map, cell partials, descriptor tables,
 * pinned host mirrors and bounce buffers -- is grow-only WHILE a call runs, so that a caller looping over frames of one size allocates once.  The
 * reference keeps nothing past the call (src/ssim.cpp:1048-1088: one alloc / dealloc pair inside compute_ssim, include/rmgr/ssim.h:505-525), so:
 *   - when a ctx == NULL call ends and its context holds more than $RMGR_SSIM_HIP_POOL_RETAIN_MB (per context, device + pinned; default 256;
 *     0: keep nothing; negative: no cap) everything is released before the context is leased again: an 8192^2 + map call (134 MB + 268 MB of
 *     staging) leaves nothing behind, a 4096^2 + map loop (100 MB) keeps its buffers;
 *   - rmgr_ssim_hip_trim_default_pool() releases the staging of every default context that is not inside a call right now (the contexts themselves --
 *     stream, events -- stay: the next call re-grows what it needs; contexts in use are skipped);
 *   - rmgr_ssim_hip_get_default_pool_memory() reports what the default contexts held when their last call ended (device bytes, pinned host bytes)
 *     and the cap in force (bytes; UINT64_MAX: none).  Any pointer may be NULL.  Creates nothing.
 * rmgr_ssim_hip_trim(ctx) does the same for a caller-owned context (which has no cap: its owner decides; it must not be in use by another
 * thread; queued work is waited for first); ctx == NULL: the default pool.  Results never depend on any of this. */
rmgr_int32_t rmgr_ssim_hip_trim_default_pool(void) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_get_default_pool_memory(rmgr_uint64_t* deviceBytes, rmgr_uint64_t* pinnedBytes, rmgr_uint64_t* retainCapBytes) RMGR_NOEXCEPT;

/* An engine instance: one device, one stream, its own grow-only scratch.  A context may be used by one
 * host thread at a time (create one per thread, or serialise); ctx == NULL entry points lease one of the
 * process-wide default contexts per call (rmgr_ssim_hip_compute_ssim_host) and may be called from any number of threads. */
typedef struct rmgr_ssim_hip_Context_ rmgr_ssim_hip_Context;

/* Number of usable HIP devices (0 when none; never fails). */
rmgr_int32_t rmgr_ssim_hip_get_device_count(rmgr_int32_t* count) RMGR_NOEXCEPT;

/* Creates an engine bound to `device`.  `stream` is a hipStream_t passed as void* (NULL: the
 * context creates and owns a non-blocking stream).  All work of the context is ordered on it. */
rmgr_int32_t rmgr_ssim_hip_create(rmgr_ssim_hip_Context** ctx, rmgr_int32_t device, void* stream) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_destroy(rmgr_ssim_hip_Context* ctx) RMGR_NOEXCEPT;

rmgr_int32_t rmgr_ssim_hip_trim(rmgr_ssim_hip_Context* ctx) RMGR_NOEXCEPT;

/* Free and total memory of the context's device in bytes (hipMemGetInfo), for hosts without a HIP runtime of their own; ctx == NULL: the device
 * of the default contexts ($RMGR_SSIM_HIP_DEVICE).  Either pointer may be NULL.  ENODEV without a device. */
rmgr_int32_t rmgr_ssim_hip_get_memory_info(const rmgr_ssim_hip_Context* ctx, rmgr_uint64_t* freeBytes, rmgr_uint64_t* totalBytes) RMGR_NOEXCEPT;

/* ctx == NULL (set and get): the arithmetic mode of the process-wide default contexts the unchanged rmgr_ssim_compute_ssim() runs on
 * (a property of their pool, applied when a call leases one: calls in flight keep theirs; neither call waits for a lease or creates a context when
 * one exists already -- only on an empty pool is the first context created, so that a machine without a device answers ENODEV).  This is what
 * rmgr::ssim::select_impl() calls (src/ssim.cpp:808-896). */
rmgr_int32_t rmgr_ssim_hip_set_mode(rmgr_ssim_hip_Context* ctx, rmgr_int32_t mode) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_get_mode(const rmgr_ssim_hip_Context* ctx, rmgr_int32_t* mode) RMGR_NOEXCEPT;

/* Tuning knobs (0 = library default): rows of the image each wavefront strip covers, and the kernel variant --
 *   1  one column per lane (64-column strips);            2  two columns per lane, row sums in the blur phase;
 *   3  two columns per lane with the bit-exact modes' (a,b) row sums formed a phase early (EARLY);
 *   6  the balanced schedule of the two-column kernel (launches without a map; modes 0, 3, 1) with the library's interleave of the images in
 *      the chunk list; 7: without any interleave (round 5's list); 100 + T: T images interleaved (measurement aids, tools/phase_ab.sh);
 * the default picks by launch size (rmgr_ssim_hip_get_plan reports what it picked; rmgr_ssim_hip_tune measures the candidates on the device).
 * Results do not depend on either (tests/test_gpu_parity.py, tests/test_gpu_pipeline.py check). */
rmgr_int32_t rmgr_ssim_hip_set_tuning(rmgr_ssim_hip_Context* ctx, rmgr_int32_t stripRows, rmgr_int32_t variant) RMGR_NOEXCEPT;

/* How a launch of `count` width x height pairs is cut into wavefront strips under the context's mode and
 * tuning (ctx may be NULL: default mode, default tuning, a 256-CU device).  Pure host arithmetic: no device
 * is touched.  The reference's counterpart is its 256x64 tile grid (src/ssim.cpp:1026-1028).
 * The caller sets plan->structSize = sizeof(rmgr_ssim_hip_Plan) BEFORE the call; the library fills the fields that fit
 * in that many bytes and nothing beyond them (EINVAL below RMGR_SSIM_HIP_PLAN_MIN_SIZE), so the struct can grow
 * without overrunning the storage of a client compiled against an earlier header. */
typedef struct rmgr_ssim_hip_Plan
{
    rmgr_uint32_t structSize;        /* in: sizeof(rmgr_ssim_hip_Plan) as the CALLER was compiled */
    rmgr_uint32_t stripWidth;        /* output columns per wavefront: 128 (two per lane) or 64 (one per lane: fp64 mode, tiny launches, tuning variant 1) */
    rmgr_uint32_t stripRows;         /* output rows per wavefront STRIP.  When balancedChunks > 0 this and the next four fields describe the strips a launch WITH a map */
    rmgr_uint32_t stripsX, stripsY;  /* strips per image                  of these pairs runs; a launch without one runs balancedChunks wavefronts of balancedChunkRows rows, */
    rmgr_uint32_t wavefronts;        /* stripsX * stripsY * count         in the EARLY form for modes 0 and 3 (128 x 1080p: 5760 strips with a map, 2041 chunks without) */
    /* -- RMGR_SSIM_HIP_PLAN_MIN_SIZE ends here -- */
    rmgr_uint32_t waveSlots;         /* wavefronts the device holds at a time with this kernel (SIMDs x waves per SIMD) */
    rmgr_uint32_t earlyRowSums;      /* 1: the bit-exact two-column kernel's STRIPS run in the EARLY form (launches of <= 3 x waveSlots wavefronts) */
    rmgr_uint32_t cellRows;          /* rows of a reduction cell (64 columns x cellRows rows): 8, or 32 for images of >= 2048 rows */
    rmgr_uint32_t cellsX, cellsY;    /* the image's grid of reduction cells: cellsX * cellsY fp64 partials per image (rmgr_ssim_hip_enqueue_rows) */
    rmgr_uint32_t balancedChunks;    /* > 0: a launch of these pairs WITHOUT a map runs the balanced schedule of the two-column kernel (modes 0, 3, 1) -- this many */
    rmgr_uint32_t balancedChunkRows; /*      wavefronts, each walking this many rows of the launch's flattened [images][strip column][row] list -- instead of */
                                     /*      the strips above (same results bit for bit; scheduling only); 0: the strips */
    rmgr_uint32_t balancedInterleave;/* round 6: images interleaved column by column in that list (1: none): neighbouring strip columns of an image stay in step */
} rmgr_ssim_hip_Plan;
#define RMGR_SSIM_HIP_PLAN_MIN_SIZE 24u
rmgr_int32_t rmgr_ssim_hip_get_plan(const rmgr_ssim_hip_Context* ctx, rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t count, rmgr_ssim_hip_Plan* plan) RMGR_NOEXCEPT;

/*
 * The plan of one launch shape, MEASURED.  rmgr_ssim_hip_get_plan reports the library's untuned default -- a model of how strips and chunks pack
 * onto the device, fitted on 256-CU MI355X boxes; rmgr_ssim_hip_tune times the candidates that model chooses between (the default; the strips at
 * the default height with the row sums in the blur phase / a phase early; half and twice the strip height; the balanced schedule where it
 * exists; the one-column kernel for small launches) on the context's own device, under the context's arithmetic mode, on synthetic pairs of
 * the shape it allocates and frees itself (distinct images up to ~1.5 GB; withMap: dense float maps; where the balanced schedule exists also the strips at its chunk
 * height), candidates interleaved over three rounds,
 * and keeps the winner for this context's later launches of exactly that shape (width, height, count, map or not, mode) while the context is
 * on its default tuning (set_tuning(ctx, 0, 0)); a winner has to beat the default by more than 0.5 %.  Results never depend on the choice.
 * Blocking (a few dozen launches of the shape).  The reference's counterpart is a caller choosing its thread count (include/rmgr/ssim.h:528-533).
 * result (may be NULL): the caller sets structSize; candidateXxx[0] is the default plan.  rmgr_ssim_hip_clear_tuned forgets every choice.
 */
#define RMGR_SSIM_HIP_TUNE_MAX_CANDIDATES 8
typedef struct rmgr_ssim_hip_TuneResult
{
    rmgr_uint32_t structSize;        /* in: sizeof(rmgr_ssim_hip_TuneResult) as the CALLER was compiled */
    rmgr_uint32_t candidates;        /* plans timed (<= RMGR_SSIM_HIP_TUNE_MAX_CANDIDATES) */
    rmgr_int32_t  bestVariant;       /* the winner as rmgr_ssim_hip_set_tuning arguments (0 / 0: the default stays) */
    rmgr_uint32_t bestStripRows;
    double        defaultMs, bestMs; /* kernel time of the default plan and of the winner: median over rounds of the mean of three launches */
    /* -- RMGR_SSIM_HIP_TUNE_RESULT_MIN_SIZE ends here -- */
    rmgr_int32_t  candidateVariant[RMGR_SSIM_HIP_TUNE_MAX_CANDIDATES];
    rmgr_uint32_t candidateStripRows[RMGR_SSIM_HIP_TUNE_MAX_CANDIDATES];
    double        candidateMs[RMGR_SSIM_HIP_TUNE_MAX_CANDIDATES];
} rmgr_ssim_hip_TuneResult;
#define RMGR_SSIM_HIP_TUNE_RESULT_MIN_SIZE 32u
rmgr_int32_t rmgr_ssim_hip_tune(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t count, rmgr_int32_t withMap,
                                rmgr_ssim_hip_TuneResult* result) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_clear_tuned(rmgr_ssim_hip_Context* ctx) RMGR_NOEXCEPT;
/* The measured choices a context holds, for hosts that tune once per machine and keep the result (a serving process that restores them at start-up pays no tuning):
 * rmgr_ssim_hip_get_tuned reads entry `index` (0, 1, ... until ENOENT) -- the launch shape (width, height, count, withMap), the arithmetic mode it was measured
 * under and the winner as rmgr_ssim_hip_set_tuning arguments; rmgr_ssim_hip_set_tuned installs (or replaces) an entry without measuring anything, for the context's CURRENT
 * mode (EINVAL for a shape with a zero dimension or count, a negative variant, or strip rows and variant both 0: that is the default, use clear_tuned).  Like every tuning it
 * changes scheduling only. */
typedef struct rmgr_ssim_hip_TunedEntry
{
    rmgr_uint32_t width, height, count;
    rmgr_int32_t  withMap, mode, variant;
    rmgr_uint32_t stripRows;
} rmgr_ssim_hip_TunedEntry;
rmgr_int32_t rmgr_ssim_hip_get_tuned(const rmgr_ssim_hip_Context* ctx, rmgr_uint32_t index, rmgr_ssim_hip_TunedEntry* entry) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_set_tuned(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t count, rmgr_int32_t withMap,
                                     rmgr_int32_t variant, rmgr_uint32_t stripRows) RMGR_NOEXCEPT;

/*
 * compute_ssim() on HOST pointers: stages both images to HBM, runs the kernels, copies the map
 * back (any ssimStep/ssimStride), returns the global SSIM.  Validation and return codes are the
 * reference's (src/ssim.cpp:962-978).  ctx may be NULL: the call then runs on one of the process-wide DEFAULT contexts
 * on device 0 (or $RMGR_SSIM_HIP_DEVICE), leased for the duration of the call.  Like the reference's function
 * (re-entrant, no global state: src/ssim.cpp:933-1106) concurrent callers run side by side -- each on a context of its
 * own (stream, staging buffers, pinned memory), one caller's copy-in under another's kernel and a third's map on its way
 * back -- up to $RMGR_SSIM_HIP_POOL calls at a time (default 4; 1 serialises them as rounds 1-4 did); further callers
 * wait for a lease.  Contexts are created on demand: a single-threaded process has one.
 * A large pair with a map is processed in row bands -- copy-in of band k+1, kernel on band k and the copy-back of
 * band k-1's map rows (by a short-lived helper thread, straight into ssimMap) overlap; the results are bit-identical
 * to the one-launch computation.  $RMGR_SSIM_HIP_BANDS overrides the band count (1: no overlap) and sends a large pair through
 * the banded path whatever its size and whether or not a map is wanted (measurement aid).
 * The calling thread's current HIP device is left as it was (true of every function in this header).
 */
rmgr_int32_t rmgr_ssim_hip_compute_ssim_host(rmgr_ssim_hip_Context* ctx, float* ssim, const rmgr_ssim_Params* params,
                                             const rmgr_ssim_ThreadPool* threadPool) RMGR_NOEXCEPT;

/*
 * Same computation with imgA.topLeft, imgB.topLeft and ssimMap being DEVICE pointers (step/stride
 * semantics unchanged).  `ssim` is a host pointer; the call returns after the result is there.
 */
rmgr_int32_t rmgr_ssim_hip_compute_ssim_device(rmgr_ssim_hip_Context* ctx, float* ssim, const rmgr_ssim_Params* params) RMGR_NOEXCEPT;

/*
 * Asynchronous batch: `count` pairs of identical width/height, all pointers device-resident.
 * One launch covers the whole batch; image i's fp64 sum of per-pixel SSIM values is written to
 * sumsDevice[i] (device memory, count doubles).  The reduction is organised in cells at fixed image positions and
 * summed in a fixed order, so the value is bit-identical however a batch is split across calls, contexts or GPUs
 * and whatever the tuning.  Different batches may be enqueued back to back: the descriptor tables are kept in a
 * small ring, nothing waits for the stream.  Returns once enqueued.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_batch(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_Params* params,
                                         double* sumsDevice) RMGR_NOEXCEPT;

/*
 * ONE image pair cut into ROW BANDS -- for an image too large, or too urgent, for one GPU ("single huge
 * image across GPUs"; the reference's counterpart is its tile grid walked by several threads, src/ssim.cpp:1048-1100).
 * Everything device-resident and asynchronous on the context's stream.
 *   rmgr_ssim_hip_enqueue_rows   computes output rows [yBegin, yBegin + yRows) of the pair (clipped to the image): the map
 *       rows of the band, if params->ssimMap is set, and the band's reduction-cell partials -- 64 columns x cellRows rows
 *       each, rmgr_ssim_hip_get_plan() reports cellRows / cellsX / cellsY -- into cellsDevice[cellY * cellsX + cellX], an
 *       array of cellsX * cellsY doubles the caller ZEROED; cells outside the band are not touched.  yBegin must be a
 *       multiple of cellRows and the band must end on one or at the last row (EINVAL otherwise).  The image pointers
 *       describe the WHOLE image (topLeft = row 0), but only source rows yBegin - 5 ... yEnd + 4 (clamped to the image)
 *       are read: a GPU that owns a band needs just those rows resident.
 *   rmgr_ssim_hip_reduce_cells   sums `count` images' complete cell arrays ([image][cellY][cellX]) into sumsDevice[image]
 *       in the fixed order every launch of this library uses.
 * Bands may be computed by different contexts or GPUs into separate zeroed arrays; adding the arrays element-wise
 * (rmgr_ssim_hip_comm_allreduce_sums on the cell array: every cell is non-zero on exactly one rank, and adding zeros is
 * exact) and reducing the result gives the SAME BITS as one launch over the whole image on one GPU.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_rows(rmgr_ssim_hip_Context* ctx, const rmgr_ssim_Params* params, rmgr_uint32_t yBegin, rmgr_uint32_t yRows,
                                        double* cellsDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_reduce_cells(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t count,
                                        const double* cellsDevice, double* sumsDevice) RMGR_NOEXCEPT;

/*
 * A batch of HOST image pairs (identical width/height, global SSIM only: every ssimMap must be NULL): what a
 * caller looping rmgr_ssim_compute_ssim() over frames does (sample/rmgr-ssim-sample.cpp:84-95, src/ssim-cli.cpp:
 * 197-210), with the staging pipelined -- pairs are copied to the GPU in chunks on a second stream while the kernels
 * of the previous chunk run, small pairs are gathered in pinned memory and sent with one DMA per chunk.  ssim[i]
 * is bit-identical to the single-pair call on pair i.  ctx may be NULL (process-wide default context).  Blocking.
 */
rmgr_int32_t rmgr_ssim_hip_compute_ssim_batch_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_Params* params,
                                                   float* ssim) RMGR_NOEXCEPT;

/*
 * The same batch of HOST pairs sharded BY IMAGE over several devices from ONE process ("one process
 * x 8 devices"): contiguous blocks of the batch -- the first count % n one pair longer -- one per entry of `devices`
 * (NULL: every visible device, deviceCount ignored), each on its own worker thread and engine context (created on first
 * use, cached), each through the pipelined staging of rmgr_ssim_hip_compute_ssim_batch_host.  No image data crosses
 * devices and, in one address space, there is no exchange step either: every ssim[i] is written by the worker that owns
 * pair i and is bit-identical to the single-device result, whatever the device list.  A device may be listed more than
 * once (several contexts on one GPU).  `mode` is the arithmetic of every worker.  Stands in for the reference's
 * thread-pool dispatch (src/ssim.cpp:1048-1088, src/ssim-openmp.c:26-47) at batch granularity.  Blocking; one call at a
 * time per process.  EINVAL for a device index that is not visible, ENODEV without devices.
 */
rmgr_int32_t rmgr_ssim_hip_compute_ssim_batch_host_devices(const rmgr_int32_t* devices, rmgr_uint32_t deviceCount, rmgr_int32_t mode,
                                                           rmgr_uint32_t count, const rmgr_ssim_Params* params, float* ssim) RMGR_NOEXCEPT;

/* ssim[i] = float(sums[i] / double(width*height)) with the reference's 32-bit product (src/ssim.cpp:1102).  Host arrays. */
rmgr_int32_t rmgr_ssim_hip_finalize(rmgr_uint32_t count, const double* sums, rmgr_uint32_t width, rmgr_uint32_t height, float* ssim) RMGR_NOEXCEPT;

/*
 * All channels of one interleaved pair (host pointers, `channelCount` bytes per pixel, rows
 * `strideA` / `strideB` bytes apart) in ONE staging copy and ONE launch: ssim[c] receives channel c's
 * global SSIM.  ssimMap (or NULL) is an interleaved float map, channelCount floats per pixel, rows
 * width*channelCount floats apart -- the layout rmgr-ssim writes (src/ssim-cli.cpp:108-127).
 */
rmgr_int32_t rmgr_ssim_hip_compute_ssim_channels_host(rmgr_ssim_hip_Context* ctx, float* ssim,
                                                      const rmgr_uint8_t* imgA, ptrdiff_t strideA, const rmgr_uint8_t* imgB, ptrdiff_t strideB,
                                                      rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t channelCount, float* ssimMap) RMGR_NOEXCEPT;

/*
 * SSIM of the BT.601 luminance of two interleaved images with >= 3 channels:
 * Y = (19595 R + 38470 G + 7471 B + 32768) / 65536 in integers (src/ssim-cli.cpp:158-186), computed on
 * the GPU from one staging copy.  ssimMap (or NULL): dense width x height floats.
 */
rmgr_int32_t rmgr_ssim_hip_compute_ssim_luminance_host(rmgr_ssim_hip_Context* ctx, float* ssim,
                                                       const rmgr_uint8_t* imgA, ptrdiff_t strideA, const rmgr_uint8_t* imgB, ptrdiff_t strideB,
                                                       rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint32_t channelCount, float* ssimMap) RMGR_NOEXCEPT;

/* The conversion alone, device to device (asynchronous on the context's stream): dstY[x + y*dstStride]
 * from src[x*srcStep + y*srcStride + {0,1,2}].  srcStep >= 3. */
rmgr_int32_t rmgr_ssim_hip_luminance_device(rmgr_ssim_hip_Context* ctx, rmgr_uint8_t* dstY, ptrdiff_t dstStride,
                                            const rmgr_uint8_t* src, ptrdiff_t srcStep, ptrdiff_t srcStride,
                                            rmgr_uint32_t width, rmgr_uint32_t height) RMGR_NOEXCEPT;

/*
 * Multi-scale SSIM (MS-SSIM; Wang, Simoncelli & Bovik, "Multi-scale structural similarity for image quality assessment", 2003) of
 * `count` uint8 pairs of one size.  No reference counterpart: the definition is pinned down here, and tests/msssim_model.py restates it
 * in float64.
 *
 *   Inputs   params[0 .. count-1]: width, height (the same for every pair), imgA / imgB with any step / stride in bytes, negative ones
 *            included.  ssimMap must be NULL (MS-SSIM has no per-pixel map); alloc / dealloc are not used.
 *   Scales   1 <= scales <= RMGR_SSIM_HIP_MSSSIM_MAX_SCALES.  Scale 0 is the input; scale s+1 is ceil(W_s/2) x ceil(H_s/2) with
 *              P_{s+1}(x,y) = ((P_s(2x,2y) + P_s(2x+1,2y)) + (P_s(2x,2y+1) + P_s(2x+1,2y+1))) * 0.25,
 *            coordinates outside scale s clamped to its last row / column (the 2x2 box filter + decimation of Wang's msssim.m; TF's
 *            symmetric pad + avg_pool).  In fp32 this pyramid is EXACT up to scale 8: scale s holds multiples of 4^-s below 256, and the
 *            sum of four needs at most 10 + 2s <= 24 significand bits.
 *   Per scale for every pixel, the blurred moments mu_a, mu_b, sigma_a^2, sigma_b^2, sigma_ab: the separable 11 + 11 tap Gaussian
 *            (sigma 1.5, normalised over the 11 taps, fp32 taps) with CLAMPED edges, as everywhere in this library, so the statistics
 *            are same-size: every pixel of the scale counts.  This differs from the "valid" window of TensorFlow's ssim_multiscale and
 *            pytorch-msssim, which drop a 5-pixel border at every scale: values are close but not equal, most of all on small scales.
 *              cs = (2 sigma_ab + C2) / (sigma_a^2 + sigma_b^2 + C2),  l = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1),  ssim = l * cs,
 *            C1 = 6.5025f, C2 = 58.5225f (the engine's).  mcs_s and mssim_s are fp64 sums of cs and ssim over the scale divided by W_s * H_s.
 *   Result   MS-SSIM = prod_{s < M-1} max(mcs_s, 0)^w_s * max(mssim_{M-1}, 0)^w_{M-1} in double (M = scales; the ReLU of TF and
 *            pytorch-msssim keeps negative means from producing NaN), returned as float in msssim[i].
 *            weights == NULL: Wang's {0.0448, 0.2856, 0.3001, 0.2363, 0.1333}, and scales must be 5.  Otherwise `scales` finite weights >= 0.
 *   Arithmetic  fp32 with centred moments as in MODE_SEPARABLE, but centred on an integer per 64 x 16 tile (the floor of the tile's
 *            middle pixel, per image) instead of 128: still exact, and much smaller cancellation on few-pixel scales.  The context's mode
 *            does not change MS-SSIM.
 *   Determinism  each image's sums run over fixed tiles of each scale in a fixed order: a pair gives the same bits alone or anywhere in a
 *            batch of any size, through either entry point, on every call.
 *   Outputs  msssim: count floats (host memory).  scaleMeans: NULL, or count x scales x 2 doubles (host memory), [image][scale]{mcs, mssim}.
 *
 * _device: the image pointers are device memory; ctx must not be NULL.  _host: host memory, copied to the device as it is (ctx NULL: a
 * default context, as rmgr_ssim_hip_compute_ssim_host).  Both block.  Device scratch: about 2.7 bytes per scale-0 pixel for the pyramid
 * (plus the staged images for _host); a batch is run in sub-batches that keep it under about 1 GB -- results do not depend on the split.
 * EINVAL: count == 0, a NULL pointer (params, msssim, an image), a zero or differing size, a non-NULL ssimMap, scales out of range, weights
 * NULL with scales != 5, a weight that is negative or not finite -- all checked before any device is touched.  ENODEV: no device.
 */
#define RMGR_SSIM_HIP_MSSSIM_MAX_SCALES 8
rmgr_int32_t rmgr_ssim_hip_compute_msssim_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_Params* params,
                                                 rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssim_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_Params* params,
                                               rmgr_uint32_t scales, const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT;

/*
 * SSIM of `count` pairs of 8- to 16-bit images of one size (10- and 12-bit video, 16-bit PNG, medical and scientific images).  No
 * reference counterpart: the definition is pinned down here, and tests/ssim16_model.py restates it in float64.
 *
 *   Samples  unsigned 16-bit, host byte order, LSB-aligned (rmgr_ssim_hip_uint16_t).  bitDepth, one value per call, 8 <= bitDepth <= 16;
 *            L = 2^bitDepth - 1.  Samples are used as stored: values above L are not rejected.  Depth 8 lets 8-bit data in 16-bit
 *            containers be cross-checked against the 8-bit engine.
 *   Inputs   params[0 .. count-1]: width, height (the same for every pair), imgA / imgB with any step / stride in SAMPLES (not bytes),
 *            negative ones included; ssimMap NULL (no map) or a float map with ssimStep / ssimStride in floats -- per pair.
 *   Constants  C1 = float((0.01 L) * (0.01 L)), C2 = float((0.03 L) * (0.03 L)), products in double: at depth 8 the engine's 6.5025f
 *            and 58.5225f.
 *   Per pixel  the blurred moments mu_a, mu_b, sigma_a^2, sigma_b^2, sigma_ab of the engine's 11-tap Gaussian (sigma 1.5, normalised
 *            over the 11 taps, fp32 taps), separable, with CLAMPED edges; variances and covariance as E[x y] - mu_x mu_y; then
 *              ssim = (2 mu_a mu_b + C1)(2 sigma_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(sigma_a^2 + sigma_b^2 + C2))
 *            (SURVEY.md A.3).
 *   Global   the mean of the per-pixel values: an fp64 sum divided by double(W) * double(H), a 64-bit product.  The 32-bit
 *            width * height of rmgr_ssim_hip_finalize (the reference's quirk) does NOT apply here.
 *   Arithmetic  fp32 with centred samples as in MODE_SEPARABLE, but the centre is an integer taken from a fixed position of the
 *            image -- A's and B's sample at (min(x0 + 64, W - 1), (H - 1) / 2) for the 128 columns from x0 = 128 k on -- so the
 *            subtraction is exact and the result does not depend on the batch.  The context's mode does not change this path.
 *   Determinism  each image's sum runs over fixed 64-column cells in a fixed order: a pair gives the same bits (value and map)
 *            alone or anywhere in a batch of any size, after any internal sub-batch split, through every entry point, on every
 *            call, and as a view with negative step or stride compared with the same pixels uploaded contiguously.
 *
 * _enqueue_ssim16: device pointers; asynchronous on the context's stream; writes each pair's fp64 SUM of per-pixel values to
 *            sumsDevice[i] (device memory), like rmgr_ssim_hip_enqueue_batch.  The mean is sum / (double(W) * double(H)).
 * _compute_ssim16_device: device pointers; blocks; ssim: count floats in host memory.
 * _compute_ssim16_host: host pointers (ctx NULL: a default context, as rmgr_ssim_hip_compute_ssim_host).  The images are staged to
 *            the device and each map is copied back at its own step and stride; a batch runs in sub-batches that keep the device
 *            scratch under about 1 GB -- results do not depend on the split.
 * EINVAL: count == 0; a NULL params, ssim, image pointer or (enqueue) sumsDevice; a zero or differing width or height, or one above
 *         0x7FFF0000; bitDepth
 *         outside 8..16; an image pointer that is not 2-byte aligned; a NULL ctx for _device or _enqueue_ssim16 -- all checked
 *         before any device is touched.  ENODEV: no device.
 */
typedef unsigned short rmgr_ssim_hip_uint16_t;
typedef struct rmgr_ssim_hip_Img16 {
    const rmgr_ssim_hip_uint16_t* topLeft;
    ptrdiff_t step, stride;                     /* in samples */
} rmgr_ssim_hip_Img16;
typedef struct rmgr_ssim_hip_Params16 {
    rmgr_uint32_t       width, height;
    rmgr_ssim_hip_Img16 imgA, imgB;
    float*              ssimMap;                /* NULL: no map */
    ptrdiff_t           ssimStep, ssimStride;   /* in floats */
} rmgr_ssim_hip_Params16;
#define RMGR_SSIM_HIP_SSIM16_MIN_DEPTH 8
#define RMGR_SSIM_HIP_SSIM16_MAX_DEPTH 16
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim16(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                          rmgr_uint32_t bitDepth, double* sumsDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssim16_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                 rmgr_uint32_t bitDepth, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssim16_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                               rmgr_uint32_t bitDepth, float* ssim) RMGR_NOEXCEPT;

/*
 * SSIM of `count` pairs of float32 images of one size, and its gradient (HDR and linear-light frames, normalised tensors, the
 * output of a model; SSIM as a training loss).  No reference counterpart: the definition is pinned down here, and
 * tests/ssimf_model.py restates it in float64, the gradient included.
 *
 *   Samples  float32 planes, used as stored.  Negative values and values above dataRange are not rejected; NaN and Inf propagate.
 *   Data range  dataRange, one float per call, finite and > 0 (R): C1 = float((0.01 R) * (0.01 R)), C2 = float((0.03 R) * (0.03 R)),
 *            products in double.
 *   Inputs   params[0 .. count-1]: width, height (the same for every pair), imgA / imgB with any step / stride in FLOATS (not bytes),
 *            negative ones included; ssimMap NULL (no map) or a float map with ssimStep / ssimStride in floats -- per pair.
 *   Window   the engine's 11-tap Gaussian (sigma 1.5, normalised over the 11 taps, fp32 taps), separable, with CLAMPED edges, same-size
 *            output: the linear operator G.
 *   Per pixel  mu_a = G a, mu_b = G b, s_aa = G(a^2) - mu_a^2, s_bb = G(b^2) - mu_b^2, s_ab = G(a b) - mu_a mu_b;
 *              A1 = 2 mu_a mu_b + C1, A2 = 2 s_ab + C2, B1 = mu_a^2 + mu_b^2 + C1, B2 = s_aa + s_bb + C2;  ssim = A1 A2 / (B1 B2).
 *   Global   S_i: the fp64 sum of the per-pixel values divided by double(W) * double(H), a 64-bit product as for ssim16.
 *   Gradient  given gOut[i] = dLoss/dS_i, the exact derivative of the above, clamped edges included.  With k = gOut[i] / (double(W) *
 *            double(H)), d_ab = 2 A1 / (B1 B2), d_aa = -ssim / B2 and
 *              d_mu = 2 mu_b A2 / (B1 B2) - 2 mu_a ssim / B1 - 2 mu_a d_aa - mu_b d_ab:
 *              dLoss/da = Gt(k d_mu) + 2 a Gt(k d_aa) + b Gt(k d_ab),    dLoss/db: the same with a and b exchanged.
 *            Gt is the ADJOINT of the clamped window, not the window: (Gt v)(q) is the sum of w_t v(p) over every (p, t) with
 *            clamp(p + t) = q.  It is separable; in the interior it equals G; the first and last row and column also collect the
 *            taps the forward pass clamped onto them: on each axis the plain blur of v zero-extended by 5, with the 5 results
 *            beyond each end added onto the end pixel.  The rule covers axes of 5 pixels and fewer, down to 1 x 1.
 *   Arithmetic  fp32 with centred samples as for ssim16: the centre of the 128 columns from x0 = 128 k on is A's and B's sample at
 *            (min(x0 + 64, W - 1), (H - 1) / 2) when its magnitude is at most dataRange, else 0.  Unlike an integer centre the
 *            subtraction rounds (to half an ulp of the difference).  The gradient kernel differentiates in the centred variables,
 *            which is the formula above with its cancelling terms removed before rounding.  The position is fixed by the image, so
 *            results do not depend on the batch.  The context's mode does not change this path.
 *   Determinism  each image's sum runs over fixed 64-column cells in a fixed order, and every gradient pixel is written by exactly one
 *            work-item in a fixed summation order (32 x 32 tiles at absolute positions, no floating-point atomics): a pair gives the
 *            same bits -- value, map, gradient -- alone or anywhere in a batch of any size, after any internal sub-batch split,
 *            through every entry point, on every call, with both gradients or one, and as a view with negative step or stride
 *            compared with the same pixels stored contiguously.
 *
 * _enqueue_ssimf: device pointers; asynchronous on the context's stream; writes each pair's fp64 SUM of per-pixel values to
 *            sumsDevice[i] (device memory).  The mean is sum / (double(W) * double(H)).
 * _compute_ssimf_device: device pointers; blocks; ssim: count floats in host memory.
 * _compute_ssimf_host: host pointers (ctx NULL: a default context, as rmgr_ssim_hip_compute_ssim_host).  The images are staged to
 *            the device and each map is copied back at its own step and stride; a batch runs in sub-batches that keep the device
 *            scratch under about 1 GB -- results do not depend on the split.
 * _enqueue_ssimf_grad: everything device-resident, asynchronous on the context's stream, no host synchronisation.  gradOutDevice:
 *            count floats in DEVICE memory (dLoss/dS_i).  gradA / gradB: arrays of count rmgr_ssim_hip_GradF (host memory) that
 *            describe where dLoss/dA and dLoss/dB of each pair go (device planes, step / stride in floats, negatives included); either
 *            array may be NULL (that gradient is not computed), not both.  Gradients are WRITTEN, not accumulated.  A gradient
 *            plane must not overlap an input plane or another gradient plane: this is not checked.  params[i].ssimMap is ignored.
 *            One fused launch recomputes the statistics: no scratch memory beyond the descriptors.
 * EINVAL: count == 0; a NULL params, ssim, image pointer, sumsDevice, gradOutDevice or gradient plane; both gradient arrays NULL; a
 *         zero or differing width or height, or one above 0x7FFF0000; a dataRange that is not finite or not > 0; an image or gradient
 *         pointer that is not 4-byte aligned; a NULL ctx for anything but _host -- all checked before any device is touched.
 *         ENODEV: no device.
 */
typedef struct rmgr_ssim_hip_ImgF {
    const float* topLeft;
    ptrdiff_t step, stride;                     /* in floats */
} rmgr_ssim_hip_ImgF;
typedef struct rmgr_ssim_hip_ParamsF {
    rmgr_uint32_t      width, height;
    rmgr_ssim_hip_ImgF imgA, imgB;
    float*             ssimMap;                 /* NULL: no map */
    ptrdiff_t          ssimStep, ssimStride;    /* in floats */
} rmgr_ssim_hip_ParamsF;
typedef struct rmgr_ssim_hip_GradF {
    float*    topLeft;
    ptrdiff_t step, stride;                     /* in floats */
} rmgr_ssim_hip_GradF;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                         float dataRange, double* sumsDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssimf_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                float dataRange, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssimf_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                              float dataRange, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                              float dataRange, const float* gradOutDevice,
                                              const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT;

/*
 * Multi-scale SSIM of `count` pairs of float32 images of one size, and its gradient (1 - MS-SSIM as a training loss; MS-SSIM of HDR,
 * linear-light and 9- to 16-bit material: uint16 converts to float32 exactly, dataRange = 2^depth - 1).  No reference counterpart:
 * the definition is pinned down here, and tests/msssimf_model.py restates it in float64, the gradient included.  Additions only:
 * RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 *   Samples, data range, inputs, window, alignment and size limit: as rmgr_ssim_hip_enqueue_ssimf (steps and strides in FLOATS;
 *            C1 = float((0.01 R)^2), C2 = float((0.03 R)^2)); params[i].ssimMap must be NULL.
 *   Scales and weights: as rmgr_ssim_hip_compute_msssim_device.  1 <= scales <= RMGR_SSIM_HIP_MSSSIM_MAX_SCALES; weights NULL: Wang's
 *            five {0.0448, 0.2856, 0.3001, 0.2363, 0.1333} and scales must be 5; else `scales` finite weights >= 0 (host memory).
 *   Pyramid  scale 0 is the input; scale s+1 is ceil(W_s/2) x ceil(H_s/2):
 *              P'(x, y) = ((P(2x, 2y) + P(2x+1, 2y)) + (P(2x, 2y+1) + P(2x+1, 2y+1))) * 0.25f,
 *            coordinates clamped to scale s, every operation rounded to fp32 in that order.  For floats the pyramid is not exact; the
 *            order is part of the definition, so the bits are reproducible.
 *   Per scale  with mu, s_aa, s_bb, s_ab, A1, A2, B1, B2 of the scale's planes as for ssimf:  cs = A2 / B2,  ssim = A1 A2 / (B1 B2);
 *            mcs_s, mssim_s: the fp64 sums of the per-pixel values divided by double(W_s) * double(H_s).
 *   Value    MS = prod_{s < M-1} max(mcs_s, 0)^w_s * max(mssim_{M-1}, 0)^w_{M-1} in double, with x^0 = 1 for every x (a zero
 *            weight switches a scale off).  A NaN mean gives a NaN value.
 *   Gradient  given gOut[i] = dLoss/dMS_i.  Let m_s be the mean scale s contributes (mcs_s, or mssim_s for the last scale).  If MS = 0
 *            (some m_s <= 0 with w_s > 0) the whole gradient is 0 (the ReLU's subgradient).  Otherwise
 *              k_s = gOut * w_s * MS / m_s / (double(W_s) * double(H_s))      (0 where w_s = 0),
 *            and the local gradient of scale s is the ssimf formula Gt(k d_mu) + 2 a Gt(k d_aa) + b Gt(k d_ab) on the scale's planes with
 *              last scale:    d_ab, d_aa, d_mu exactly as for ssimf;
 *              other scales:  d_ab = 2 / B2,  d_aa = -cs / B2,  d_mu = -2 mu_a d_aa - mu_b d_ab      (cs only).
 *            The total runs from the coarsest scale down through the ADJOINT of the clamped box filter:
 *              g_s(x, y) = local_s(x, y) + 0.25 * c(x, y) * g_{s+1}(x >> 1, y >> 1),    c = cx * cy,
 *            cx = 2 on the last column of an odd W_s (the column the clamp read twice; W_s = 1 included), else 1; likewise cy.
 *            A gather: one writer per pixel, no atomics.  g_0 is dLoss/da (dLoss/db: a and b exchanged).
 *   Arithmetic  fp32, centred at EVERY scale by the ssimf rule applied to that scale's planes: the centre of the 128 columns from
 *            x0 = 128 k on is A's and B's sample of scale s at (min(x0 + 64, W_s - 1), (H_s - 1) / 2) when its magnitude is at most
 *            dataRange, else 0.  The position is fixed by the image, so results do not depend on the batch.  k_s is rounded to float
 *            once; 0.25 c is a power of two, so g_s = fp32(local_s + fp32(0.25 c g_{s+1})) adds one rounding per scale.  A scale
 *            whose k_s is 0 contributes +0 whatever its samples are.  The product, the ReLU and k_s are computed on the device (pow
 *            in double).  The context's mode does not change this path.
 *   Determinism  as for ssimf: value, per-scale means and gradients have the same bits alone or anywhere in a batch, after any
 *            sub-batch split, through every entry point, on every call, with one gradient or both, and for views with negative steps
 *            or interleaved samples against the same pixels stored contiguously.  No floating-point atomics.
 *
 * _enqueue_msssimf: device pointers; asynchronous on the context's stream, never waits for the host.  valuesDevice: count doubles
 *            (MS_i); scaleMeansDevice: count x scales x 2 doubles, [pair][scale]{mcs, mssim} -- both in DEVICE memory, both required.
 * _compute_msssimf_device: device pointers; blocks.  msssim: count floats (host memory); scaleMeans: NULL, or count x scales x 2
 *            doubles (host memory).
 * _compute_msssimf_host: host pointers (ctx NULL: a default context); the images are staged to the device.
 * _enqueue_msssimf_grad: everything device-resident, asynchronous on the context's stream, no host synchronisation.
 *            scaleMeansDevice: what the forward wrote for the same pairs, scales and weights (16 x scales bytes per pair is all a
 *            training step has to keep besides its inputs); gradOutDevice: count floats (device); gradA / gradB as for
 *            _enqueue_ssimf_grad (either may be NULL, not both; written, not accumulated, each pixel once).  The pyramid is recomputed,
 *            the forward statistics are not redone.
 * Scratch  belongs to the context and is reused in stream order: the pyramid planes of scales >= 1 (about 2.7 bytes per scale-0 pixel of
 *            a pair) and, in the backward, the gradient planes of scales >= 1 (up to 2.7 bytes more).  A batch runs in sub-batches
 *            that keep it under about 1 GB; results do not depend on the split.
 * EINVAL: every EINVAL of rmgr_ssim_hip_enqueue_ssimf / _enqueue_ssimf_grad and of rmgr_ssim_hip_compute_msssim_device (scales out of
 *         range, NULL weights with scales != 5, a negative or non-finite weight, a non-NULL ssimMap), a NULL valuesDevice,
 *         scaleMeansDevice or msssim -- all checked before any device is touched.  ENODEV: no device.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_msssimf(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                           float dataRange, rmgr_uint32_t scales, const double* weights,
                                           double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssimf_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                  float dataRange, rmgr_uint32_t scales, const double* weights,
                                                  float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssimf_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                float dataRange, rmgr_uint32_t scales, const double* weights,
                                                float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_msssimf_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                float dataRange, rmgr_uint32_t scales, const double* weights,
                                                const double* scaleMeansDevice, const float* gradOutDevice,
                                                const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT;

/*
 * SSIM of `count` pairs of float16 or bfloat16 images of one size, and its gradient (what a model produces under mixed precision; SSIM
 * as a training loss without a float32 copy of the images or of the gradient).  No reference counterpart: the definition is
 * rmgr_ssim_hip_enqueue_ssimf's on the samples widened to float32, so tests/ssimf_model.py restates it as well; tests/halfmodel.py
 * restates the two encodings.  Additions only: RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 *   Samples  16-bit, host byte order (rmgr_ssim_hip_uint16_t), in ONE encoding per call: sampleType RMGR_SSIM_HIP_SAMPLE_F16 (IEEE
 *            binary16) or RMGR_SSIM_HIP_SAMPLE_BF16 (bfloat16: the upper half of a float32).  Each sample is widened to float32
 *            EXACTLY: float16 subnormals become the float32 normals they equal (they are not flushed), a bfloat16 sample is the
 *            float32 whose upper 16 bits it is, NaN and Inf stay NaN and Inf.  The widened samples are used as stored, as for ssimf.
 *   Data range, window, per pixel, global, constants  as rmgr_ssim_hip_enqueue_ssimf, word for word, on the widened planes: dataRange
 *            finite and > 0, C1 = float((0.01 R) * (0.01 R)), C2 = float((0.03 R) * (0.03 R)), the clamped 11-tap window G, the
 *            per-pixel formula, S_i = the fp64 sum of the per-pixel values divided by double(W) * double(H).
 *   Inputs   params[0 .. count-1] (rmgr_ssim_hip_Params16): width, height (the same for every pair), imgA / imgB with any step / stride
 *            in SAMPLES (not bytes), negative ones included; ssimMap NULL (no map) or a FLOAT32 map with ssimStep / ssimStride in
 *            floats -- per pair.
 *   Arithmetic  ssimf's: fp32 with centred samples, the centre of the 128 columns from x0 = 128 k on being A's and B's WIDENED sample
 *            at (min(x0 + 64, W - 1), (H - 1) / 2) when its magnitude is at most dataRange, else 0 (a NaN counts as `else`); the same
 *            64-column cells and the same 32 x 32 gradient tiles at absolute positions.  Value, map and every per-image sum have the
 *            BITS rmgr_ssim_hip_enqueue_ssimf / _compute_ssimf_* give on the widened planes.  The context's mode does not change this
 *            path.
 *   Gradient  the float32 value rmgr_ssim_hip_enqueue_ssimf_grad would store for the widened planes, rounded ONCE, to nearest-even, into
 *            the sample encoding of the inputs.  float16 results below the normal range are kept as subnormals (not flushed), overflow
 *            gives +-Inf; NaN stays NaN, its payload is not specified.  gOut stays float32, so a loss scale that arrives in gOut is
 *            applied before the single rounding.  The gradient of a mean is of order gOut / (W H): in float16 it underflows for all
 *            but small images unless gOut carries a loss scale.  float32 gradient planes for 16-bit inputs are not offered.
 *   Determinism  everything ssimf promises: the same bits -- value, map, gradient -- alone or anywhere in a batch of any size, after any
 *            internal sub-batch split, through every entry point, on every call, with both gradients or one, and as a view with
 *            negative step or stride, or interleaved samples, compared with the same pixels stored contiguously.  One writer per
 *            gradient pixel, no atomics.
 *
 * _enqueue_ssimh: device pointers; asynchronous on the context's stream, never waits for the host; writes each pair's fp64 SUM of
 *            per-pixel values to sumsDevice[i] (device memory).  The mean is sum / (double(W) * double(H)).
 * _compute_ssimh_device: device pointers; blocks; ssim: count floats in host memory.
 * _compute_ssimh_host: host pointers (ctx NULL: a default context, as rmgr_ssim_hip_compute_ssim_host).  The images are staged to
 *            the device and each map is copied back at its own step and stride; a batch runs in sub-batches that keep the device
 *            scratch under about 1 GB -- results do not depend on the split.
 * _enqueue_ssimh_grad: everything device-resident, asynchronous on the context's stream, no host synchronisation.  gradOutDevice:
 *            count FLOAT32 values in DEVICE memory (dLoss/dS_i).  gradA / gradB: arrays of count rmgr_ssim_hip_GradH (host memory) that
 *            describe where dLoss/dA and dLoss/dB of each pair go (16-bit device planes in the inputs' encoding, step / stride in
 *            samples, negatives included); either array may be NULL (that gradient is not computed), not both.  Gradients are WRITTEN,
 *            not accumulated.  A gradient plane must not overlap an input plane or another gradient plane: this is not checked.
 *            params[i].ssimMap is ignored.  One fused launch recomputes the statistics: no scratch memory beyond the descriptors.
 * EINVAL: count == 0; a NULL params, ssim, image pointer, sumsDevice, gradOutDevice or gradient plane; both gradient arrays NULL; a
 *         zero or differing width or height, or one above 0x7FFF0000; a dataRange that is not finite or not > 0; a sampleType that is
 *         neither of the two constants; an image or gradient pointer that is not 2-byte aligned; a NULL ctx for anything but _host --
 *         all checked before any device is touched.  ENODEV: no device.
 */
#define RMGR_SSIM_HIP_SAMPLE_F16  0   /* IEEE 754 binary16 */
#define RMGR_SSIM_HIP_SAMPLE_BF16 1   /* bfloat16 */
typedef struct rmgr_ssim_hip_GradH {
    rmgr_ssim_hip_uint16_t* topLeft;
    ptrdiff_t step, stride;                     /* in samples */
} rmgr_ssim_hip_GradH;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                         rmgr_uint32_t sampleType, float dataRange, double* sumsDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssimh_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                rmgr_uint32_t sampleType, float dataRange, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssimh_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                              rmgr_uint32_t sampleType, float dataRange, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                              rmgr_uint32_t sampleType, float dataRange, const float* gradOutDevice,
                                              const rmgr_ssim_hip_GradH* gradA, const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT;

/*
 * Multi-scale SSIM of `count` pairs of float16 or bfloat16 images of one size, and its gradient (1 - MS-SSIM as a training loss under
 * mixed precision, without a float32 copy of the images or of the gradient).  No reference counterpart: msssimh is msssimf applied to the
 * samples widened to float32, so tests/msssimf_model.py restates it as well; tests/halfmodel.py restates the two encodings.  Additions
 * only: RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 *   Samples  as rmgr_ssim_hip_enqueue_ssimh: 16-bit, ONE encoding per call (sampleType RMGR_SSIM_HIP_SAMPLE_F16 or _BF16), each widened
 *            to float32 EXACTLY (float16 subnormals are kept; NaN and Inf stay NaN and Inf).  Only scale 0 holds 16-bit samples: the
 *            pyramid is float32 from scale 1 on.
 *   Inputs   params[0 .. count-1] (rmgr_ssim_hip_Params16): width, height (the same for every pair), imgA / imgB with any step / stride
 *            in SAMPLES, negative and interleaved views included; params[i].ssimMap must be NULL.  Alignment: 2 bytes.
 *   Data range, scales, weights, pyramid, per scale, value, arithmetic  as rmgr_ssim_hip_enqueue_msssimf, word for word, on the widened
 *            planes.
 *   Forward  the value and every per-scale mean {mcs_s, mssim_s} have the BITS rmgr_ssim_hip_enqueue_msssimf gives on the widened planes,
 *            at every `scales` 1 .. 8 and with any weights.
 *   Gradient  the float32 value rmgr_ssim_hip_enqueue_msssimf_grad would store at scale 0 for the widened planes -- fp32(local_0 +
 *            fp32(0.25 c g_1)) when a coarser scale exists, local_0 when scales == 1 --, rounded ONCE, to nearest-even, into the inputs'
 *            encoding.  float16 keeps subnormals and overflows to +-Inf; a NaN stays a (quiet) NaN.  gradOutDevice, the per-scale means,
 *            the coefficients k_s and the gradient planes of scales >= 1 stay float32 / float64 as they are; a loss scale that arrives
 *            in gOut is applied before the single rounding.
 *   Determinism  every promise of msssimf: the same bits -- value, means, gradient -- alone or anywhere in a batch, after any sub-batch
 *            split, through every entry point, on every call, with one gradient or both, and as a view with negative step or stride, or
 *            interleaved samples, compared with the same pixels stored contiguously.  One writer per gradient pixel, no floating-point
 *            atomics.
 *
 * _enqueue_msssimh, _compute_msssimh_device, _compute_msssimh_host: as the msssimf entries of the same names (valuesDevice,
 *            scaleMeansDevice, msssim, scaleMeans as there); the _host form stages 2 bytes per pixel.
 * _enqueue_msssimh_grad: as _enqueue_msssimf_grad; gradA / gradB: arrays of count rmgr_ssim_hip_GradH as for _enqueue_ssimh_grad (16-bit
 *            device planes in the inputs' encoding, step / stride in samples; either may be NULL, not both; written, not accumulated).
 * Scratch  msssimf's: the pyramids and the coarse gradient planes are the same float32 planes; the same sub-batches under about 1 GB.
 * EINVAL: every EINVAL of the msssimf entries -- count == 0, a NULL pointer, a zero, differing or too large size, a bad dataRange, scales
 *         or weights, a non-NULL ssimMap, a NULL ctx for anything but _host --, a sampleType that is neither of the two constants, an
 *         image or gradient pointer that is not 2-byte aligned -- all checked before any device is touched.  ENODEV: no device.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_msssimh(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                           rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                           double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssimh_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                  rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                  float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssimh_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_msssimh_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                const double* scaleMeansDevice, const float* gradOutDevice,
                                                const rmgr_ssim_hip_GradH* gradA, const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT;

/*
 * Gradient of the SSIM map: dLoss/da and dLoss/db of `count` pairs for an upstream gradient given PER PIXEL (a weighted or masked mean,
 * a per-pixel combination with L1 and a minimum over views, sums over boxes -- any loss that is a function of the map
 * rmgr_ssim_hip_enqueue_ssimf / _ssimh write through params[i].ssimMap, not of its plain mean).  No reference counterpart:
 * tests/ssimw_model.py restates it in float64.  Additions only: RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 * It is the definition of rmgr_ssim_hip_enqueue_ssimf_grad with ONE change:
 *   Input    per pair a float32 plane gMap_i(p) = dLoss/dssim_i(p) in place of the scalar gOut[i]: k(p) = gMap_i(p).  There is no
 *            division by W H.
 *   Gradient  dLoss/da = Gt(k d_mu) + 2 a Gt(k d_aa) + b Gt(k d_ab) with k INSIDE Gt (it multiplies d_* at the pixel p of the map, before
 *            the adjoint spreads them);  dLoss/db: the same with a and b exchanged.
 *   Everything else is ssimf's, word for word: samples, dataRange and the constants, the window G, the clamped edges and their adjoint
 *            Gt, the centring per 128-column strip column, d_mu, d_aa, d_ab in the centred variables, 32 x 32 tiles at absolute positions
 *            with one writer per gradient pixel and no floating-point atomics.
 *   Products  k(p) d(p) is a plain fp32 product.  A zero weight does not hide a NaN or Inf statistic: 0 * NaN is NaN, and it reaches the up
 *            to 11 x 11 gradient pixels whose window holds p.  Mask such samples out of the images, not only out of gMap.
 *   Identity  for a plane gMap_i whose every element is the float  float(double(gOut[i]) / (double(W) * double(H)))  the gradients have
 *            the BITS rmgr_ssim_hip_enqueue_ssimf_grad stores for gOut[i]; for 16-bit samples, those of rmgr_ssim_hip_enqueue_ssimh_grad.
 *   float16 / bfloat16 samples (_ssimh_map_grad)  as rmgr_ssim_hip_enqueue_ssimh: the gradient is the float32 value of the widened planes,
 *            rounded ONCE, to nearest-even, into the inputs' encoding (subnormals kept, overflow to Inf, NaN stays NaN).  gMap stays
 *            float32, so a loss scale that arrives in it is applied before the single rounding.
 *   Determinism  as for ssimf: the same bits alone or anywhere in a batch, after any sub-batch split, on every call, with one gradient
 *            or both, and for negative-step or interleaved views of the samples, of gMap or of the gradient planes compared with the
 *            same pixels stored contiguously.
 *
 * gradOutMaps: an array of count rmgr_ssim_hip_GradOutF in HOST memory, each describing a plane in DEVICE memory: gMap_i(x, y) is
 *            topLeft[x * step + y * stride], step and stride in floats, negatives and 0 included -- with step = stride = 0 one float
 *            stands for the whole plane (what a framework hands over as the expanded gradient of a mean).
 * gradA / gradB: as for _enqueue_ssimf_grad / _enqueue_ssimh_grad (either may be NULL, not both).  Gradients are WRITTEN, not accumulated.  A
 *            gradient plane must not overlap an input plane, a gMap plane or another gradient plane: this is not checked.
 *            params[i].ssimMap is ignored.  Everything is device-resident; the call is asynchronous on the context's stream and never
 *            waits for the host.  One fused launch recomputes the statistics: no scratch memory beyond the descriptors.
 * The arguments before gradOutMaps are those of the corresponding _grad entry, in its order (sampleType before dataRange for 16-bit samples).
 * EINVAL: every EINVAL of rmgr_ssim_hip_enqueue_ssimf_grad / _enqueue_ssimh_grad, a NULL gradOutMaps, a gMap topLeft that is NULL or not
 *         4-byte aligned -- all checked before any device is touched.  ENODEV: no device.
 */
typedef struct rmgr_ssim_hip_GradOutF {
    const float* topLeft;
    ptrdiff_t    step, stride;                  /* in floats; 0 allowed */
} rmgr_ssim_hip_GradOutF;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf_map_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                  float dataRange, const rmgr_ssim_hip_GradOutF* gradOutMaps,
                                                  const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh_map_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                  rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_GradOutF* gradOutMaps,
                                                  const rmgr_ssim_hip_GradH* gradA, const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT;

/*
 * SSIM of float32 samples under a caller-chosen WINDOW: the five entries of the float32 family -- _enqueue_ssimf, _compute_ssimf_device,
 * _compute_ssimf_host, _enqueue_ssimf_grad, _enqueue_ssimf_map_grad -- with one more argument, `window`, after dataRange.  What other
 * libraries call win_size / win_sigma, kernel_size / sigma, filter_size / filter_sigma or window_size, and the 7 x 7 or 3 x 3 box of
 * skimage and of monodepth-style photometric losses.  No reference counterpart: tests/ssimk_model.py restates it in float64.  Additions
 * only: RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 *   Window   size is 3, 5, 7, 9 or 11 taps per axis; R = (size - 1) / 2.
 *            GAUSSIAN  sigma is finite and > 0.  With s = double(sigma): g_i = exp(-(i i) / (2 s s)) for i = 0 .. R; the norm is accumulated
 *                      in double in the order i = 0 .. R, g_0 once and the others twice; tap i is float(g_i / norm).
 *                      {11, GAUSSIAN, 1.5f} yields the engine's taps bit for bit.
 *            UNIFORM   every tap is float(1.0 / size) (a box); sigma is ignored.
 *            A NULL window means {11, GAUSSIAN, 1.5f}: the entry without _win, with its bits.
 *   Everything else is the text of the entry without _win with 5 replaced by R: the window is separable, edges are clamped, the output has
 *            the input's size; the per-pixel formula, C1 and C2 from dataRange, the fp64 sum over double(W) * double(H); the gradient with
 *            Gt, the adjoint of the clamped window -- the R results beyond each end fold onto the end pixel: tail[d] = g_d + ... + g_R and
 *            the total of all taps are summed in double and rounded once, and the rule holds for axes shorter than the window, down to
 *            1 x 1 --; the centre of every 128-column strip column at the same position with the same |c| <= dataRange test; fp32
 *            arithmetic, the row pass centre tap first with folded symmetric sums, then the column pass in source-row order; 64-column
 *            cells, 32 x 32 gradient tiles at absolute positions, one writer per pixel, no floating-point atomics; and every determinism
 *            promise of ssimf.  For the map gradient: a plane of float(double(gOut[i]) / (double(W) * double(H))) gives the bits of
 *            _enqueue_ssimf_win_grad for gOut[i] under the same window.
 *   Reach    a window reads nothing beyond its radius: a NaN sample makes NaN exactly the map pixels within R of it on both axes (edge
 *            clamping taken into account) and the gradient pixels within 2R; it is not a zero-padded 11-tap window.
 *   Borders  box windows here CLAMP where monodepth-style code reflects: the interior is identical, the outermost R pixels differ.
 *   Accuracy measured per window against the float64 model: tests/ssimk_model.py (EMU_*, *_TOL) and DESIGN.md section 16.
 *
 * Arguments, EINVAL / ENODEV rules, sub-batches, scratch and stream behaviour are those of the entry without _win.  Additional EINVAL,
 * checked before any device is touched: a size outside the five, an unknown kind, a Gaussian sigma that is not finite or not > 0.
 *
 * float16 / bfloat16 samples under a caller-chosen window: the ssimh_win entries, below.  Multi-scale SSIM of float32 and 16-bit
 * samples under a caller-chosen window: the msssimf_win and msssimh_win entries, further below.
 */
enum { RMGR_SSIM_HIP_WINDOW_GAUSSIAN = 0, RMGR_SSIM_HIP_WINDOW_UNIFORM = 1 };
typedef struct rmgr_ssim_hip_Window {
    rmgr_uint32_t size, kind;                   /* taps per axis: 3, 5, 7, 9 or 11; RMGR_SSIM_HIP_WINDOW_* */
    float         sigma;                        /* GAUSSIAN: finite, > 0; UNIFORM: ignored */
} rmgr_ssim_hip_Window;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf_win(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                             float dataRange, const rmgr_ssim_hip_Window* window, double* sumsDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssimf_win_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                    float dataRange, const rmgr_ssim_hip_Window* window, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssimf_win_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                  float dataRange, const rmgr_ssim_hip_Window* window, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf_win_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                  float dataRange, const rmgr_ssim_hip_Window* window, const float* gradOutDevice,
                                                  const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimf_win_map_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                      float dataRange, const rmgr_ssim_hip_Window* window, const rmgr_ssim_hip_GradOutF* gradOutMaps,
                                                      const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT;

/*
 * SSIM of float16 / bfloat16 samples under a caller-chosen WINDOW: the five entries of the 16-bit family -- _enqueue_ssimh,
 * _compute_ssimh_device, _compute_ssimh_host, _enqueue_ssimh_grad, _enqueue_ssimh_map_grad -- with one more argument, `window`, after
 * dataRange: the rmgr_ssim_hip_Window of the float32 _win entries, unchanged.  What a 2-D model trained under mixed precision needs when
 * its loss is the 3 x 3 box of monodepth-style photometric losses, skimage's 7 x 7 box or another size or sigma: the 16-bit tensors are
 * read as they are stored, without float32 copies and without a float32 gradient.  No reference counterpart.  Additions only:
 * RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 * It is the definition of rmgr_ssim_hip_enqueue_ssimf_win -- and of _enqueue_ssimf_win_grad and _enqueue_ssimf_win_map_grad --, word for
 * word, on samples widened to float32 exactly as the ssimh entries define widening:
 *   Window   size 3, 5, 7, 9 or 11 taps on both axes, GAUSSIAN of any finite sigma > 0 or UNIFORM; the taps of the float32 _win entries,
 *            bit for bit.  A NULL window means {11, GAUSSIAN, 1.5f}.
 *   Value    the value, the float32 map and every per-image fp64 sum have the BITS rmgr_ssim_hip_enqueue_ssimf_win gives on the widened
 *            planes under the same window.
 *   Gradient  each gradient pixel is the float32 value _enqueue_ssimf_win_grad / _enqueue_ssimf_win_map_grad would store for the widened
 *            planes under the same window, rounded ONCE, to nearest-even, into the inputs' encoding (float16: subnormals are kept,
 *            overflow gives Inf; NaN stays NaN in both encodings).  gradOutDevice and rmgr_ssim_hip_GradOutF stay float32: a loss scale
 *            arrives before the single rounding.
 *   Identity with the fixed-window entries  a NULL window and {11, GAUSSIAN, 1.5f} give the BITS of the ssimh entries without _win:
 *            value, map, sums and both gradient forms.
 *   Identity of the two gradient forms  a gMap whose every element is float(double(gOut[i]) / (double(W) * double(H))) gives the BITS of
 *            _enqueue_ssimh_win_grad for gOut[i] under the same window.
 *   Everything else is ssimf_win's: determinism (alone or anywhere in a batch, at any strip height, after any sub-batch split, as any
 *            view), the clamped borders, the centre of every 128-column strip column, and the reach of a NaN sample ((2R + 1)^2 map
 *            pixels, (4R + 1)^2 gradient pixels, clipped) and of a NaN in gMap ((2R + 1)^2).
 *
 * Arguments, strides (in 16-bit samples; the map and gMap in floats), EINVAL / ENODEV rules, sub-batches, scratch and stream behaviour are
 * those of the ssimh entry without _win.  Additional EINVAL, checked after that entry's sample type, data range and pairs, before its
 * upstream and gradient planes and before any device is touched: a size outside the five, an unknown kind, a Gaussian sigma that is not
 * finite or not > 0.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh_win(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                             rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                             double* sumsDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssimh_win_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                    rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                    float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssimh_win_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                  rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                  float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh_win_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                  rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                  const float* gradOutDevice, const rmgr_ssim_hip_GradH* gradA,
                                                  const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssimh_win_map_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                      rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                      const rmgr_ssim_hip_GradOutF* gradOutMaps, const rmgr_ssim_hip_GradH* gradA,
                                                      const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT;

/*
 * MULTI-SCALE SSIM of float32 and of float16 / bfloat16 samples under a caller-chosen WINDOW: the four entries of each multi-scale
 * family -- _enqueue_msssimf, _compute_msssimf_device, _compute_msssimf_host, _enqueue_msssimf_grad and their msssimh counterparts --
 * with one more argument, `window`, after dataRange: the rmgr_ssim_hip_Window of the single-scale _win entries, unchanged.  What
 * pytorch-msssim calls ms_ssim(win_size, win_sigma), torchmetrics kernel_size / sigma, TensorFlow filter_size / filter_sigma.  No
 * reference counterpart: tests/msssimk_model.py restates it in float64, the gradient included.  Additions only:
 * RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 * It is the definition of rmgr_ssim_hip_enqueue_msssimf / _enqueue_msssimf_grad (of _enqueue_msssimh / _enqueue_msssimh_grad) with 5
 * replaced by R = (size - 1) / 2 AT EVERY SCALE:
 *   Window   size 3, 5, 7, 9 or 11 taps on both axes, GAUSSIAN of any finite sigma > 0 or UNIFORM; the taps of the single-scale _win
 *            entries, bit for bit.  The SAME window -- size and taps -- applies to every scale of the pyramid, as in pytorch-msssim; it
 *            is not rescaled with the planes.  A NULL window means {11, GAUSSIAN, 1.5f}.
 *   Per scale  mu, s_aa, s_bb, s_ab of a scale's planes are those of rmgr_ssim_hip_enqueue_ssimf_win under the window: separable, edges
 *            clamped.  A coarse plane smaller than the window clamps like any other, down to 1 x 1: every tap then reads the same few
 *            samples and the adjoint's tails (tail[d] = g_d + ... + g_R, summed in double and rounded once) fold onto them.
 *   Unchanged, word for word  the pyramid and its rounding order; C1 and C2; cs = A2 / B2 and ssim = A1 A2 / (B1 B2); the fp64 means over
 *            double(W_s) * double(H_s); the ReLU'd weighted product in double; k_s; the local gradient Gt(k d_mu) + 2 a Gt(k d_aa) +
 *            b Gt(k d_ab) with Gt the adjoint of the clamped window; the adjoint of the clamped box filter, 0.25 c g_{s+1}(x >> 1, y >> 1),
 *            one more rounding per scale; the centre of every 128-column strip column of each scale with its |c| <= dataRange test;
 *            +0 from a scale whose k_s is 0.  None of them depends on the radius.
 *   16-bit samples  as the msssimh entries define them: the value and every per-scale mean have the BITS of the msssimf_win entry on the
 *            widened planes under the same window; each gradient pixel is the float32 value _enqueue_msssimf_win_grad would store for
 *            the widened planes, rounded ONCE, to nearest-even, into the inputs' encoding.  gradOutDevice stays float32.
 *   Identity with the fixed-window entries  a NULL window and {11, GAUSSIAN, 1.5f} give the BITS of the entries without _win: values,
 *            per-scale means and gradients.
 *   Determinism  every promise of msssimf / msssimh: the same bits alone or anywhere in a batch, after any sub-batch split, through every
 *            entry point, on every call, with one gradient or both, and for any view of the same pixels.  No floating-point atomics.
 *   Reach    a window reads nothing beyond its radius at any scale; it is not a zero-padded 11-tap window.
 *   Accuracy measured per window against the float64 model: tests/msssimk_model.py (EMU) and DESIGN.md section 26.
 *
 * Arguments, EINVAL / ENODEV rules, sub-batches, scratch (it does not depend on the window) and stream behaviour are those of the entry
 * without _win.  Additional EINVAL, checked after that entry's data range, pairs, scales and weights, before its other pointers and before
 * the context or any device is touched: a size outside the five, an unknown kind, a Gaussian sigma that is not finite or not > 0.
 *
 * Not in this interface: the uint8 multi-scale entries (rmgr_ssim_hip_compute_msssim_*) keep the reference's window.  Multi-scale SSIM
 * of volumes under a caller-chosen window: the msssim3f_win and msssim3h_win entries, last of the volume entries.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_msssimf_win(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                               float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                               const double* weights, double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssimf_win_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                      float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                      const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssimf_win_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                    float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                    const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_msssimf_win_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_ParamsF* params,
                                                    float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                    const double* weights, const double* scaleMeansDevice, const float* gradOutDevice,
                                                    const rmgr_ssim_hip_GradF* gradA, const rmgr_ssim_hip_GradF* gradB) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_msssimh_win(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                               rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                               rmgr_uint32_t scales, const double* weights, double* valuesDevice,
                                               double* scaleMeansDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssimh_win_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                      rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                      rmgr_uint32_t scales, const double* weights, float* msssim,
                                                      double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssimh_win_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                    rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                    rmgr_uint32_t scales, const double* weights, float* msssim,
                                                    double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_msssimh_win_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params16* params,
                                                    rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                    rmgr_uint32_t scales, const double* weights, const double* scaleMeansDevice,
                                                    const float* gradOutDevice, const rmgr_ssim_hip_GradH* gradA,
                                                    const rmgr_ssim_hip_GradH* gradB) RMGR_NOEXCEPT;

/*
 * SSIM of `count` pairs of float32 VOLUMES of one size under a THREE-DIMENSIONAL window, and its gradient (MRI / CT reconstruction,
 * volumetric super-resolution, spatio-temporal video losses): what pytorch-msssim computes with spatial_dims = 3, torchmetrics on 5-D
 * input, MONAI's SSIMLoss(spatial_dims = 3) and skimage on n-D arrays.  The 2-D entries on a stack of slices compute independent 2-D
 * SSIMs with no window across slices; this family is not that.  No reference counterpart: the definition is pinned down here, and
 * tests/ssim3f_model.py restates it in float64, the gradient included.  Additions only: RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 *   Samples  float32 volumes, used as stored.  Negative values and values above dataRange are not rejected; NaN and Inf propagate.
 *   Data range  dataRange, one float per call, finite and > 0 (R): C1 and C2 exactly as for rmgr_ssim_hip_enqueue_ssimf.
 *   Inputs   params[0 .. count-1]: width, height, depth (the same for every pair, each 1 .. 0x7FFF0000); voxel (x, y, z) of A is
 *            imgA.topLeft[x * step + y * stride + z * sliceStride], in FLOATS, each a signed ptrdiff_t of any value, negatives and 0
 *            included; ssimMap NULL (no map) or a float volume addressed the same way by ssimStep / ssimStride / ssimSliceStride -- per
 *            pair.  Every offset is a 64-bit product: volumes whose slices lie more than 2^32 bytes apart work.
 *   Window   the engine's 11-tap Gaussian (sigma 1.5, the fp32 taps of every other entry), separable over x, y and z, with CLAMPED edges
 *            on every axis, same-size output: the linear operator G.
 *   Per voxel  the formulas of rmgr_ssim_hip_enqueue_ssimf with this G: mu_a = G a, mu_b = G b, s_aa = G(a^2) - mu_a^2, s_bb = G(b^2) -
 *            mu_b^2, s_ab = G(a b) - mu_a mu_b; A1 = 2 mu_a mu_b + C1, A2 = 2 s_ab + C2, B1 = mu_a^2 + mu_b^2 + C1, B2 = s_aa + s_bb + C2;
 *            ssim = A1 A2 / (B1 B2).
 *   Global   S_i: the fp64 sum of the per-voxel values divided by double(W) * double(H) * double(D).
 *   Gradient  given gOut[i] = dLoss/dS_i, the exact derivative of the above, clamped edges included.  With k = float(double(gOut[i]) /
 *            (double(W) * double(H) * double(D))) and ssimf's d_ab = 2 A1 / (B1 B2), d_aa = -ssim / B2,
 *              d_mu = 2 mu_b A2 / (B1 B2) - 2 mu_a ssim / B1 - 2 mu_a d_aa - mu_b d_ab:
 *              dLoss/da = Gt(k d_mu) + 2 a Gt(k d_aa) + b Gt(k d_ab),    dLoss/db: the same with a and b exchanged.
 *            Gt is the ADJOINT of the clamped 3-D window.  It is separable; on each axis it is ssimf's rule: the plain blur of v
 *            zero-extended by 5, with the 5 results beyond each end added onto the end voxel.  The rule holds down to 1 x 1 x 1.
 *   Arithmetic  fp32 with centred samples, a' = a - cA, b' = b - cB.  ONE centre per volume (not one per 128 columns as in 2-D): A's and
 *            B's sample at ((W - 1) / 2, (H - 1) / 2, (D - 1) / 2), used when its magnitude is at most dataRange, else 0.  It depends on
 *            the volume alone.  (One centre for the whole volume lets the backward keep coefficients of the centred variables: a
 *            coefficient and the voxel that collects it always share their centre.)  The x pass runs centre tap first on folded symmetric
 *            sums, the y pass and the z pass in source order, the first product plain and the others fused; the gradient differentiates in
 *            the centred variables, as ssimf's.  The context's mode does not change this path.
 *   Determinism  each volume's sum runs over fixed cells of 16 x 16 x 8 voxels at absolute positions in a fixed order, and every map and
 *            gradient voxel is written by exactly one work-item in a fixed summation order; the order does not depend on how a launch is cut
 *            into tiles, z-chunks or sub-batches; no floating-point atomics.  A pair gives the same bits -- value, map, gradients -- alone or
 *            anywhere in a batch, on every call, through every entry point, with one gradient or both, and as any view (negative or
 *            permuted strides, interleaved samples) compared with the same voxels stored densely.
 *   Reach    a NaN voxel makes NaN exactly the 11 x 11 x 11 map voxels and the 21 x 21 x 21 gradient voxels around it, clipped to the volume
 *            (clamping taken into account); everything else stays finite (a NaN at the centre position makes the centre 0).
 *
 * _enqueue_ssim3f: device pointers; asynchronous on the context's stream, never waits for the host; writes each pair's fp64 SUM of
 *            per-voxel values to sumsDevice[i] (device memory).
 * _compute_ssim3f_device: device pointers; blocks; ssim: count floats in host memory.
 * _compute_ssim3f_host: host pointers (ctx NULL: a default context).  The volumes are staged to the device and each map is copied back at
 *            its own strides; a batch runs in sub-batches that keep the device scratch under about 1 GB, at least one volume each.
 * _enqueue_ssim3f_grad: everything device-resident, asynchronous on the context's stream, no host synchronisation.  gradOutDevice: count
 *            floats in DEVICE memory.  gradA / gradB: arrays of count rmgr_ssim_hip_Grad3F (host memory); either may be NULL, not both.
 *            Gradients are WRITTEN, not accumulated.  A gradient volume must not overlap an input or another gradient volume: not checked.
 *            params[i].ssimMap is ignored.
 *            Scratch: a first walk writes the weighted partial derivatives k d_mu, k d_aa, k d_ab of every voxel -- 12 bytes per voxel for
 *            one gradient, 16 for both (d_mu differs, d_aa and d_ab are shared) -- into the context's scratch, a second walk applies Gt.
 *            The scratch belongs to the context and is reused in stream order; a batch runs in sub-batches of about 1 GB of it, at least one
 *            volume each (a volume of 512^3 takes 2 GB for both gradients).
 * EINVAL: count == 0; a NULL params, ssim, volume pointer, sumsDevice, gradOutDevice or gradient volume; both gradient arrays NULL; a zero
 *         or differing width, height or depth, or one above 0x7FFF0000; a volume with more than 2^24 - 1 tiles of 16 x 16 columns; a
 *         dataRange that is not finite or not > 0; a volume, map or gradient pointer that is not 4-byte aligned; a NULL ctx for anything
 *         but _host -- all checked before any device is touched.  ENODEV: no device.
 *
 * Follow-ups, not in this interface: a caller-chosen window (the _win entries), float16 / bfloat16 volumes and multi-scale SSIM of
 * volumes.  (The 16-bit volumes have since arrived under the ssim3h names, below, the caller-chosen window for float32 volumes
 * under the ssim3f_win names and the one for 16-bit volumes under the ssim3h_win names, both further below, and multi-scale SSIM of
 * float32 volumes under the msssim3f names, last of the volume entries.)
 */
typedef struct rmgr_ssim_hip_Img3F {
    const float* topLeft;
    ptrdiff_t step, stride, sliceStride;        /* in floats */
} rmgr_ssim_hip_Img3F;
typedef struct rmgr_ssim_hip_Params3F {
    rmgr_uint32_t       width, height, depth;
    rmgr_ssim_hip_Img3F imgA, imgB;
    float*              ssimMap;                /* NULL: no map */
    ptrdiff_t           ssimStep, ssimStride, ssimSliceStride;    /* in floats */
} rmgr_ssim_hip_Params3F;
typedef struct rmgr_ssim_hip_Grad3F {
    float*    topLeft;
    ptrdiff_t step, stride, sliceStride;        /* in floats */
} rmgr_ssim_hip_Grad3F;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                          float dataRange, double* sumsDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                 float dataRange, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                               float dataRange, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                               float dataRange, const float* gradOutDevice,
                                               const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT;

/*
 * Gradient of the 3-D SSIM map: dLoss/da and dLoss/db of `count` pairs of float32 volumes for an upstream gradient given PER VOXEL (SSIM
 * inside a brain or body mask, validity or saliency weights of a spatio-temporal loss, a per-voxel combination with L1 -- any loss that
 * is a function of the map rmgr_ssim_hip_enqueue_ssim3f writes through params[i].ssimMap, not of its plain mean).  No reference
 * counterpart: tests/ssim3w_model.py restates it in float64.  Additions only: RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 * It is the definition of rmgr_ssim_hip_enqueue_ssim3f_grad with ONE change:
 *   Input    per pair a float32 volume gMap_i(p) = dLoss/dssim_i(p) in place of the scalar gOut[i]: k(p) = gMap_i(p).  There is no
 *            division by W H D.
 *   Gradient  dLoss/da = Gt(k d_mu) + 2 a Gt(k d_aa) + b Gt(k d_ab) with k INSIDE Gt (it multiplies d_* at the voxel p of the map, before
 *            the adjoint spreads them);  dLoss/db: the same with a and b exchanged.
 *   Everything else is ssim3f's, word for word: samples, dataRange and the constants, the window G over x, y and z, the clamped edges on
 *            all three axes and their adjoint Gt, ONE centre per volume, d_mu, d_aa, d_ab in the centred variables, the summation
 *            orders, one writer per gradient voxel and no floating-point atomics, and the scratch: the first walk stores k d_mu, k d_aa,
 *            k d_ab -- 12 bytes per voxel for one gradient, 16 for both -- into the context's scratch, which it shares with
 *            _enqueue_ssim3f_grad in stream order, and a batch runs in sub-batches of about 1 GB of it, at least one volume each.
 *   Products  k(p) d(p) is a plain fp32 product.  A zero weight does not hide a NaN or Inf in the images: 0 * NaN is NaN.  Mask such
 *            samples out of the volumes, not only out of gMap.
 *   Reach    a NaN in gMap at p makes NaN exactly the 11 x 11 x 11 gradient voxels around p, clipped to the volume; a NaN sample reaches
 *            21 x 21 x 21 as before.
 *   Identity  for a volume gMap_i whose every element is the float  float(double(gOut[i]) / (double(W) * double(H) * double(D)))  the
 *            gradients have the BITS rmgr_ssim_hip_enqueue_ssim3f_grad stores for gOut[i].
 *   Determinism  as for ssim3f, extended to views of gMap: the same bits alone or anywhere in a batch, at any z-chunk depth and after
 *            any sub-batch split, on every call, with one gradient or both, and for any view (negative, permuted, interleaved or zero
 *            strides) of the samples, of gMap or of the gradient volumes compared with the same voxels stored densely.
 *
 * gradOutMaps: an array of count rmgr_ssim_hip_GradOut3F in HOST memory, each describing a volume in DEVICE memory: gMap_i(x, y, z) is
 *            topLeft[x * step + y * stride + z * sliceStride], in floats, negatives and 0 included, every offset a 64-bit product -- with
 *            all three 0 one float stands for the whole volume (what a framework hands over as the expanded gradient of a sum).
 * gradA / gradB: as for _enqueue_ssim3f_grad (either may be NULL, not both).  Gradients are WRITTEN, not accumulated.  A gradient volume
 *            must not overlap an input volume, a gMap volume or another gradient volume: this is not checked.  params[i].ssimMap is
 *            ignored.  Everything is device-resident; the call is asynchronous on the context's stream and never waits for the host.
 * EINVAL: every EINVAL of rmgr_ssim_hip_enqueue_ssim3f_grad, a NULL gradOutMaps, a gMap topLeft that is NULL or not 4-byte aligned -- all
 *         checked before any device is touched.  ENODEV: no device.
 */
typedef struct rmgr_ssim_hip_GradOut3F {
    const float* topLeft;
    ptrdiff_t    step, stride, sliceStride;     /* in floats; negatives and 0 allowed */
} rmgr_ssim_hip_GradOut3F;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_map_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                   float dataRange, const rmgr_ssim_hip_GradOut3F* gradOutMaps,
                                                   const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT;

/*
 * SSIM of float32 VOLUMES under a caller-chosen WINDOW: the five entries of the float32 volume family -- _enqueue_ssim3f,
 * _compute_ssim3f_device, _compute_ssim3f_host, _enqueue_ssim3f_grad, _enqueue_ssim3f_map_grad -- with one more argument, `window`, after
 * dataRange: the rmgr_ssim_hip_Window of the 2-D _win entries, unchanged.  What MONAI, torchmetrics and pytorch-msssim call win_size /
 * kernel_size / sigma with spatial_dims = 3, and the 7-tap box skimage applies to n-D arrays; the window for volumes that are thin along
 * one axis (clips of 8 to 16 frames, slabs of a few slices), where an 11-tap clamped window is mostly border.  No reference counterpart:
 * tests/ssim3k_model.py restates it in float64.  Additions only: RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 *   Window   size is 3, 5, 7, 9 or 11 taps on ALL THREE axes (the window is isotropic); R = (size - 1) / 2.  The taps are those of the 2-D
 *            _win entries, bit for bit: GAUSSIAN taps normalised in double in the order i = 0 .. R, a UNIFORM tap float(1.0 / size).
 *            A NULL window means {11, GAUSSIAN, 1.5f}.
 *   Everything else is the text of rmgr_ssim_hip_enqueue_ssim3f (and _ssim3f_grad, _ssim3f_map_grad) with 5 replaced by R: clamped edges
 *            on every axis and same-size output; ONE centre per volume; the x pass centre tap first on folded symmetric sums, the y pass
 *            and the z pass in source order with the first product plain; fp32 arithmetic without contraction; fixed cells of 16 x 16 x 8
 *            voxels at absolute positions, one writer per voxel, no floating-point atomics; 12 / 16 bytes per voxel of coefficient scratch
 *            in sub-batches of about 1 GB; 64-bit offsets and arbitrary signed strides; Gt, the adjoint of the clamped window -- the R
 *            results beyond each end fold onto the end voxel: tail[d] = g_d + ... + g_R and the total of all taps are summed in double and
 *            rounded once --, down to 1 x 1 x 1.
 *   Identity with the fixed-window entries  {11, GAUSSIAN, 1.5f} and a NULL window give the BITS of the entries without _win: value, map,
 *            sums and both gradient forms.
 *   Identity of the two gradient forms  a gMap whose every element is float(double(gOut[i]) / (double(W) * double(H) * double(D))) gives the
 *            BITS of _enqueue_ssim3f_win_grad for gOut[i] under the same window.
 *   Determinism  that of ssim3f: the same bits alone or anywhere in a batch, at any z-chunk depth and after any sub-batch split, on every
 *            call, through every entry point, with one gradient or both, and for any view compared with the same voxels stored densely.
 *   Reach    a window reads nothing beyond its radius: a NaN sample makes NaN exactly the (2R + 1)^3 map voxels and the (4R + 1)^3
 *            gradient voxels around it, clipped to the volume (clamping taken into account); a NaN in gMap reaches (2R + 1)^3 gradient
 *            voxels.  A window of 3 taps is not a zero-padded 11-tap window.
 *   Borders  box windows here CLAMP at the borders where skimage and monodepth-style code reflect or crop: the interior is identical, the
 *            outermost R voxels of every axis differ.
 *   Accuracy measured per window against the float64 model: tests/ssim3k_model.py (EMU_*, TOL_FACTOR) and DESIGN.md section 21.
 *
 * Arguments, EINVAL / ENODEV rules, sub-batches, scratch and stream behaviour are those of the entry without _win.  Additional EINVAL,
 * checked before any device is touched: a size outside the five, an unknown kind, a Gaussian sigma that is not finite or not > 0.
 *
 * float16 / bfloat16 volumes under a caller-chosen window: the ssim3h_win entries, below.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_win(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                              float dataRange, const rmgr_ssim_hip_Window* window, double* sumsDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_win_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                     float dataRange, const rmgr_ssim_hip_Window* window, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssim3f_win_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                   float dataRange, const rmgr_ssim_hip_Window* window, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_win_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                   float dataRange, const rmgr_ssim_hip_Window* window, const float* gradOutDevice,
                                                   const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3f_win_map_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                       float dataRange, const rmgr_ssim_hip_Window* window, const rmgr_ssim_hip_GradOut3F* gradOutMaps,
                                                       const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT;

/*
 * SSIM of `count` pairs of float16 / bfloat16 VOLUMES of one size under the three-dimensional window, its gradient and the gradient of its
 * map: the volumes a model produces under mixed precision, read as they are stored.  No reference counterpart.  Additions only:
 * RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 * It is the definition of rmgr_ssim_hip_enqueue_ssim3f -- and of _enqueue_ssim3f_grad and _enqueue_ssim3f_map_grad --, word for word, on
 * samples widened to float32 exactly as rmgr_ssim_hip_enqueue_ssimh defines widening:
 *   Samples  16-bit, host byte order (rmgr_ssim_hip_uint16_t), in ONE encoding per call: sampleType RMGR_SSIM_HIP_SAMPLE_F16 (IEEE
 *            binary16) or RMGR_SSIM_HIP_SAMPLE_BF16 (bfloat16: the upper half of a float32).  Each sample is widened to float32 exactly:
 *            float16 subnormals are kept, NaN and Inf stay NaN and Inf.  Negative values and values above dataRange are not rejected.
 *   Value    the value, the float32 map and every per-volume fp64 sum have the BITS rmgr_ssim_hip_enqueue_ssim3f gives on the widened
 *            volumes.  The ONE centre per volume is the widened centre sample, used when its magnitude is at most dataRange, else 0.
 *   Gradient  each gradient voxel is the float32 value rmgr_ssim_hip_enqueue_ssim3f_grad would store for the widened volumes, rounded ONCE, to
 *            nearest-even, into the inputs' encoding (float16: subnormals are kept, overflow gives Inf; NaN stays NaN in both encodings).
 *            For _enqueue_ssim3h_map_grad the float32 value is _enqueue_ssim3f_map_grad's.  gradOutDevice and the upstream volumes
 *            (rmgr_ssim_hip_GradOut3F, reused as it is) stay float32: a loss scale arrives before the single rounding.
 *   Identity  for a volume gMap_i whose every element is the float  float(double(gOut[i]) / (double(W) * double(H) * double(D)))
 *            _enqueue_ssim3h_map_grad stores the BITS of _enqueue_ssim3h_grad for gOut[i].
 *   Everything else is ssim3f's: the window, the clamped edges and their adjoint, the arithmetic and its summation orders, the cells of
 *            16 x 16 x 8 voxels, determinism (alone or anywhere in a batch, at any z-chunk depth, after any sub-batch split, as any view),
 *            the reach of a NaN sample (11 x 11 x 11 map voxels, 21 x 21 x 21 gradient voxels, clipped) and of a NaN in gMap (11 x 11 x
 *            11), and the scratch: the coefficient volumes stay float32, 12 bytes per voxel for one gradient and 16 for both, in the
 *            scratch the float32 entries use, in sub-batches of about 1 GB of it, at least one volume each.
 *
 * Inputs: params[0 .. count-1] as for ssim3f; imgA / imgB steps, strides and slice strides count 16-bit SAMPLES (signed, 0 included); the
 * map is float32 and its strides count floats.  The entries are those of ssim3f with sampleType after params: _enqueue_ssim3h (device
 * pointers, asynchronous, fp64 sums into sumsDevice), _compute_ssim3h_device (device pointers, blocks), _compute_ssim3h_host (host
 * pointers, ctx NULL: a default context; 2 bytes per sample are staged and each float32 map is copied back at its own strides),
 * _enqueue_ssim3h_grad and _enqueue_ssim3h_map_grad (device-resident, asynchronous; gradA / gradB: arrays of count rmgr_ssim_hip_Grad3H
 * in host memory, either may be NULL, not both; gradients are WRITTEN, not accumulated, and must not overlap an input, a gMap or each
 * other: not checked; params[i].ssimMap is ignored).
 * EINVAL: everything rmgr_ssim_hip_enqueue_ssim3f / _ssim3f_grad / _ssim3f_map_grad refuse, with 2-byte alignment in place of 4-byte
 *         alignment for the sample and gradient pointers (the map and gMap stay 4-byte aligned), and a sampleType that is neither of the
 *         two constants -- all checked before any device is touched.  ENODEV: no device.
 */
typedef struct rmgr_ssim_hip_Img3H {
    const rmgr_ssim_hip_uint16_t* topLeft;
    ptrdiff_t step, stride, sliceStride;        /* in 16-bit samples */
} rmgr_ssim_hip_Img3H;
typedef struct rmgr_ssim_hip_Params3H {
    rmgr_uint32_t       width, height, depth;
    rmgr_ssim_hip_Img3H imgA, imgB;
    float*              ssimMap;                /* NULL: no map */
    ptrdiff_t           ssimStep, ssimStride, ssimSliceStride;    /* in floats */
} rmgr_ssim_hip_Params3H;
typedef struct rmgr_ssim_hip_Grad3H {
    rmgr_ssim_hip_uint16_t* topLeft;
    ptrdiff_t step, stride, sliceStride;        /* in 16-bit samples */
} rmgr_ssim_hip_Grad3H;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                          rmgr_uint32_t sampleType, float dataRange, double* sumsDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssim3h_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                 rmgr_uint32_t sampleType, float dataRange, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssim3h_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                               rmgr_uint32_t sampleType, float dataRange, float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                               rmgr_uint32_t sampleType, float dataRange, const float* gradOutDevice,
                                               const rmgr_ssim_hip_Grad3H* gradA, const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h_map_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                   rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_GradOut3F* gradOutMaps,
                                                   const rmgr_ssim_hip_Grad3H* gradA, const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT;

/*
 * SSIM of float16 / bfloat16 VOLUMES under a caller-chosen WINDOW: the five entries of the 16-bit volume family -- _enqueue_ssim3h,
 * _compute_ssim3h_device, _compute_ssim3h_host, _enqueue_ssim3h_grad, _enqueue_ssim3h_map_grad -- with one more argument, `window`, after
 * dataRange: the rmgr_ssim_hip_Window of the float32 _win entries, unchanged.  What a volumetric model trained under mixed precision
 * needs when its clips or slabs are thin along one axis, or when its metric is MONAI's, torchmetrics' or skimage's 7-tap window: the
 * 16-bit tensors are read as they are stored, without float32 copies and without a float32 gradient.  No reference counterpart.
 * Additions only: RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 * It is the definition of rmgr_ssim_hip_enqueue_ssim3f_win -- and of _enqueue_ssim3f_win_grad and _enqueue_ssim3f_win_map_grad --, word
 * for word, on samples widened to float32 exactly as the ssim3h entries define widening:
 *   Window   size 3, 5, 7, 9 or 11 taps on all three axes, GAUSSIAN of any finite sigma > 0 or UNIFORM; the taps of the float32 _win
 *            entries, bit for bit.  A NULL window means {11, GAUSSIAN, 1.5f}.
 *   Value    the value, the float32 map and every per-volume fp64 sum have the BITS rmgr_ssim_hip_enqueue_ssim3f_win gives on the widened
 *            volumes under the same window.
 *   Gradient  each gradient voxel is the float32 value _enqueue_ssim3f_win_grad / _enqueue_ssim3f_win_map_grad would store for the widened
 *            volumes under the same window, rounded ONCE, to nearest-even, into the inputs' encoding (float16: subnormals are kept,
 *            overflow gives Inf; NaN stays NaN in both encodings).  gradOutDevice and rmgr_ssim_hip_GradOut3F stay float32: a loss scale
 *            arrives before the single rounding.
 *   Identity with the fixed-window entries  a NULL window and {11, GAUSSIAN, 1.5f} give the BITS of the ssim3h entries without _win:
 *            value, map, sums and both gradient forms.
 *   Identity of the two gradient forms  a gMap whose every element is float(double(gOut[i]) / (double(W) * double(H) * double(D))) gives the
 *            BITS of _enqueue_ssim3h_win_grad for gOut[i] under the same window.
 *   Everything else is ssim3f_win's: determinism (alone or anywhere in a batch, at any z-chunk depth, after any sub-batch split, as any
 *            view), the reach of a NaN sample ((2R + 1)^3 map voxels, (4R + 1)^3 gradient voxels, clipped) and of a NaN in gMap
 *            ((2R + 1)^3), the clamped borders, and the scratch: float32 coefficient volumes, 12 / 16 bytes per voxel, in the scratch the
 *            float32 entries use, in sub-batches of about 1 GB of it.
 *
 * Arguments, strides (in 16-bit samples; the map and gMap in floats), EINVAL / ENODEV rules, sub-batches, scratch and stream behaviour are
 * those of the ssim3h entry without _win.  Additional EINVAL, checked after that entry's and before any device is touched: a size outside
 * the five, an unknown kind, a Gaussian sigma that is not finite or not > 0.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h_win(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                              rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                              double* sumsDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssim3h_win_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                     rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                     float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_ssim3h_win_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                   rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                   float* ssim) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h_win_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                   rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                   const float* gradOutDevice, const rmgr_ssim_hip_Grad3H* gradA,
                                                   const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_ssim3h_win_map_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                       rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                       const rmgr_ssim_hip_GradOut3F* gradOutMaps, const rmgr_ssim_hip_Grad3H* gradA,
                                                       const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT;

/*
 * Multi-scale SSIM (MS-SSIM) of `count` pairs of float32 VOLUMES of one size, and its gradient.  No reference counterpart.  It is the
 * definition of rmgr_ssim_hip_enqueue_msssimf carried to three axes, with the per-voxel terms of rmgr_ssim_hip_enqueue_ssim3f; float32
 * and the engine's 11-tap window only.
 *
 *   Samples, addressing, data range, C1 / C2, size limit, alignment  as rmgr_ssim_hip_enqueue_ssim3f: Params3F, signed strides of any
 *            kind, 64-bit offsets.  params[i].ssimMap must be NULL.
 *   Scales and weights  as rmgr_ssim_hip_enqueue_msssimf: 1 <= scales <= RMGR_SSIM_HIP_MSSSIM_MAX_SCALES; weights NULL: Wang's five
 *            {0.0448, 0.2856, 0.3001, 0.2363, 0.1333}, and then scales must be 5; otherwise `scales` finite weights >= 0 in HOST memory.
 *   Pyramid  scale 0 is the input.  Scale s+1 is ceil(W_s/2) x ceil(H_s/2) x ceil(D_s/2), coordinates clamped to scale s:
 *              P'(x,y,z) = (((P(2x,2y,2z) + P(2x+1,2y,2z)) + (P(2x,2y+1,2z) + P(2x+1,2y+1,2z))) +
 *                           ((P(2x,2y,2z+1) + P(2x+1,2y,2z+1)) + (P(2x,2y+1,2z+1) + P(2x+1,2y+1,2z+1)))) * 0.125f,
 *            every operation rounded to fp32 in that order.  All three axes are halved (avg_pool3d of pytorch-msssim does the same); an
 *            axis that has reached 1 stays 1, so the pyramid runs down to 1 x 1 x 1.
 *   Per scale  with ssim3f's A1, A2, B1, B2 under the 11-tap Gaussian clamped on all three axes: cs = A2 / B2, ssim = A1 A2 / (B1 B2);
 *            mcs_s and mssim_s are the fp64 sums of the fp32 values over double(W_s) * double(H_s) * double(D_s).  Both are reported for
 *            every scale, whatever its weight.
 *   Value    MS = prod_{s < M-1} max(mcs_s, 0)^w_s * max(mssim_{M-1}, 0)^w_{M-1}, in double on the device, x^0 = 1.  A NaN mean gives NaN.
 *   Gradient  for gOut[i] = dLoss/dMS_i.  All +0 when MS = 0, and when gOut[i] = 0 whatever the samples are.  Otherwise, with m_s = mcs_s (mssim_s on the last scale),
 *              k_s = float((((double(gOut) * w_s) * MS) / m_s) / (double(W_s) * double(H_s) * double(D_s))),
 *            in that order, rounded once, and 0 where w_s = 0.  The local gradient of scale s is Gt(k d_mu) + 2 a Gt(k d_aa) + b Gt(k d_ab)
 *            with ssim3f's partial derivatives on the last scale and the cs form on the others: d_ab = 2 / B2, d_aa = -cs / B2,
 *            d_mu = -2 mu_a d_aa - mu_b d_ab.  The total is
 *              g_s(x,y,z) = fp32(local_s + fp32(0.125 c g_{s+1}(x >> 1, y >> 1, z >> 1))),   c = cx cy cz,
 *            cx = 2 on the last column of an odd W_s (1 included), else 1; cy and cz likewise; 0.125 c is a power of two, so the product is
 *            exact.  A scale whose k_s is 0 for a volume contributes +0 whatever its samples are, NaN included: decided on the device, no
 *            host wait.  A gather: one writer per voxel, no floating-point atomics.  Gradients are written, not accumulated; either of
 *            gradA / gradB may be NULL, not both.  The backward recomputes the pyramid, not the means: scaleMeansDevice is the forward's.
 *   Arithmetic  fp32 with one centre per volume AT EVERY SCALE: the scale's own sample at ((W_s-1)/2, (H_s-1)/2, (D_s-1)/2) when its
 *            magnitude is at most dataRange, else 0.  Cells are 16 x 16 x 8 at absolute positions of each scale, summed in a fixed tree.
 *   Determinism  ssim3f's, for value, per-scale means and gradients: the same bits alone or anywhere in a batch, at any z-chunk depth of
 *            any scale, after any sub-batch split, through every entry, with one gradient or both, for any view against the dense volume.
 *   Identities  mssim_s has the BITS of rmgr_ssim_hip_enqueue_ssim3f's per-volume sum on the scale-s volume, divided by its voxel count in
 *            double.  With scales = 1 and weights = {1} the gradient has the BITS of rmgr_ssim_hip_enqueue_ssim3f_map_grad under a
 *            zero-stride gMap holding k_0.
 *   Scratch  belongs to the context and is reused in stream order.  The pyramid volumes of scales >= 1 take about 8/7 bytes per scale-0
 *            voxel of a pair; in the backward the coarse gradient volumes take 4/7 (one gradient) or 8/7 (both) bytes more; ssim3f's
 *            coefficient volumes take 12 / 16 bytes per voxel of the LARGEST scale and are reused by every scale.  A batch runs in
 *            sub-batches of about 1 GB of it, at least one volume each.
 *   scaleMeans  [pair][scale]{mcs, mssim}: count x scales x 2 doubles; may be NULL for compute_*, not for enqueue.
 *
 * EINVAL, before any device is touched: every EINVAL of the ssim3f entries and of msssimf's scales / weights checks; a non-NULL ssimMap;
 * a NULL msssim, valuesDevice, scaleMeansDevice or gradOutDevice; a volume whose first pyramid step alone needs 2^32 work-items.
 * ENODEV: no device.
 *
 * Against pytorch-msssim's MS_SSIM(spatial_dims=3): that one uses a valid window and zero-padded pooling and refuses small sides; this
 * one clamps the window at the borders, pools with clamped coordinates and runs down to 1 x 1 x 1, so values are close, not equal.
 *
 * float16 / bfloat16 volumes: the msssim3h entries below.  A caller-chosen window for the multi-scale form: the msssim3f_win and
 * msssim3h_win entries, further below.  Follow-up, not in this interface: a multi-scale map gradient.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3f(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                            float dataRange, rmgr_uint32_t scales, const double* weights, double* valuesDevice,
                                            double* scaleMeansDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssim3f_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                   float dataRange, rmgr_uint32_t scales, const double* weights, float* msssim,
                                                   double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssim3f_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                 float dataRange, rmgr_uint32_t scales, const double* weights, float* msssim,
                                                 double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3f_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                 float dataRange, rmgr_uint32_t scales, const double* weights, const double* scaleMeansDevice,
                                                 const float* gradOutDevice, const rmgr_ssim_hip_Grad3F* gradA,
                                                 const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT;

/*
 * Multi-scale SSIM of `count` pairs of float16 or bfloat16 VOLUMES of one size, and its gradient (1 - MS-SSIM of volumes as a training
 * loss under mixed precision, without a float32 copy of the volumes or of the gradient).  No reference counterpart: msssim3h is msssim3f
 * applied to the samples widened to float32, so tests/msssim3f_model.py restates it as well; tests/halfmodel.py restates the two
 * encodings.  Additions only: RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 *   Samples  as rmgr_ssim_hip_enqueue_ssim3h: 16-bit, ONE encoding per call (sampleType RMGR_SSIM_HIP_SAMPLE_F16 or _BF16), each widened
 *            to float32 EXACTLY (float16 subnormals are kept; bfloat16 is the upper half of a float32; NaN and Inf stay NaN and Inf).
 *            Only scale 0 holds 16-bit samples: the pyramid is float32 from scale 1 on.
 *   Inputs   params[0 .. count-1] (rmgr_ssim_hip_Params3H): width, height, depth (the same for every pair), imgA / imgB with any step /
 *            stride / sliceStride in SAMPLES, negative and interleaved views included, 64-bit offsets; params[i].ssimMap must be NULL.
 *            Alignment: 2 bytes.
 *   Data range, scales, weights, pyramid, per scale, value, arithmetic  as rmgr_ssim_hip_enqueue_msssim3f, word for word, on the widened
 *            volumes.
 *   Forward  the value and every per-scale mean {mcs_s, mssim_s} have the BITS rmgr_ssim_hip_enqueue_msssim3f gives on the widened
 *            volumes, at every `scales` 1 .. 8 and with any weights.
 *   Gradient  the float32 value rmgr_ssim_hip_enqueue_msssim3f_grad would store at scale 0 for the widened volumes -- fp32(local_0 +
 *            fp32(0.125 c g_1)) when a coarser scale exists, local_0 when scales == 1 --, rounded ONCE, to nearest-even, into the inputs'
 *            encoding.  float16 keeps subnormals and overflows to +-Inf; a NaN stays a (quiet) NaN.  gradOutDevice, the per-scale means,
 *            the coefficients k_s, the pyramid, the gradient volumes of scales >= 1 and the coefficient volumes stay float32 / float64
 *            as they are; a loss scale that arrives in gOut is applied before the single rounding: round(scale g), not scale round(g).
 *            A volume whose k_0 is 0 (a zero weight, MS = 0 or gOut = 0) stores the rounded upstream share fp32(0.125 c g_1) at scale 0:
 *            +0 when scales == 1.
 *   Determinism  every promise of msssim3f: the same bits -- value, means, gradient -- alone or anywhere in a batch, at any z-chunk depth
 *            of any scale, after any sub-batch split, through every entry point, with one gradient or both, and for any view against
 *            the dense volume.  One writer per gradient voxel, no floating-point atomics.
 *
 * _enqueue_msssim3h, _compute_msssim3h_device, _compute_msssim3h_host: as the msssim3f entries of the same names (valuesDevice,
 *            scaleMeansDevice, msssim, scaleMeans as there); the _host form stages 2 bytes per voxel.
 * _enqueue_msssim3h_grad: as _enqueue_msssim3f_grad; gradA / gradB: arrays of count rmgr_ssim_hip_Grad3H as for _enqueue_ssim3h_grad
 *            (16-bit device volumes in the inputs' encoding, step / stride / sliceStride in samples; either may be NULL, not both;
 *            written, not accumulated).
 * Scratch  msssim3f's, byte for byte: the pyramids, the coarse gradient volumes and the coefficient volumes are the same float32 volumes,
 *            in the same sub-batches under about 1 GB.
 * EINVAL, before any device is touched: every EINVAL of the msssim3f entries, with 2-byte alignment for samples and gradient volumes in
 *         place of 4; a sampleType that is neither of the two constants.  ENODEV: no device.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3h(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                            rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                            double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssim3h_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                   rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                   float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssim3h_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                 rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                 float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3h_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                 rmgr_uint32_t sampleType, float dataRange, rmgr_uint32_t scales, const double* weights,
                                                 const double* scaleMeansDevice, const float* gradOutDevice,
                                                 const rmgr_ssim_hip_Grad3H* gradA, const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT;

/*
 * MULTI-SCALE SSIM of float32 and of float16 / bfloat16 VOLUMES under a caller-chosen WINDOW: the four entries of each multi-scale
 * volume family -- _enqueue_msssim3f, _compute_msssim3f_device, _compute_msssim3f_host, _enqueue_msssim3f_grad and their msssim3h
 * counterparts -- with one more argument, `window`, after dataRange: the rmgr_ssim_hip_Window of the single-scale _win entries,
 * unchanged.  What pytorch-msssim calls MS_SSIM(spatial_dims=3, win_size, win_sigma); MONAI and torchmetrics expose the same window.  No
 * reference counterpart: tests/msssim3k_model.py restates it in float64, the gradient included.  Additions only:
 * RMGR_SSIM_HIP_ABI_VERSION stays 6.
 *
 * It is the definition of rmgr_ssim_hip_enqueue_msssim3f / _enqueue_msssim3f_grad (of _enqueue_msssim3h / _enqueue_msssim3h_grad) with 5
 * replaced by R = (size - 1) / 2 ON EVERY AXIS AT EVERY SCALE:
 *   Window   size 3, 5, 7, 9 or 11 taps on all three axes, GAUSSIAN of any finite sigma > 0 or UNIFORM; the taps of
 *            rmgr_ssim_hip_enqueue_ssim3f_win, bit for bit.  The SAME window -- size and taps -- applies to every scale of the pyramid, as
 *            in pytorch-msssim; it is not rescaled with the volumes.  A NULL window means {11, GAUSSIAN, 1.5f}.
 *   Per scale  mu, s_aa, s_bb, s_ab of a scale's volumes are those of rmgr_ssim_hip_enqueue_ssim3f_win under the window: separable, edges
 *            clamped.  A coarse volume smaller than the window clamps like any other, down to 1 x 1 x 1: every tap then reads the same
 *            few samples and the adjoint's tails (tail[d] = g_d + ... + g_R, summed in double and rounded once) fold onto them.  The
 *            pyramid halves all three axes, so a 12-frame clip has depth 12, 6, 3, 2, 1: from scale 2 on an 11-tap window is nothing but
 *            border along z, which is what a window of 7 or 3 taps is for.
 *   Unchanged, word for word  the clamped 2 x 2 x 2 pyramid and its fp32 order; C1 and C2; cs = A2 / B2 and ssim = A1 A2 / (B1 B2); the
 *            fp64 means over double(W_s) * double(H_s) * double(D_s); the ReLU'd weighted product in double; k_s; the local gradient
 *            Gt(k d_mu) + 2 a Gt(k d_aa) + b Gt(k d_ab) with Gt the adjoint of the clamped window; the adjoint of the clamped box filter,
 *            0.125 c g_{s+1}(x >> 1, y >> 1, z >> 1), one more rounding per scale; one centre per volume per scale with its |c| <=
 *            dataRange test; the 16 x 16 x 8 cells at absolute positions; +0 from a scale whose k_s is 0.  None of them depends on the
 *            radius.
 *   16-bit samples  as the msssim3h entries define them: the value and both means of every scale have the BITS of the msssim3f_win entry
 *            on the exactly widened volumes under the same window; each gradient voxel is the float32 value _enqueue_msssim3f_win_grad
 *            would store for the widened volumes, rounded ONCE, to nearest-even, into the inputs' encoding.  There is no tolerance in
 *            this contract.  gradOutDevice stays float32, so a loss scale arrives before the single rounding.
 *   Identity with the fixed-window entries  a NULL window and {11, GAUSSIAN, 1.5f} give the BITS of the entries without _win: values,
 *            per-scale means and gradients.
 *   Determinism  every promise of msssim3f / msssim3h: the same bits alone or anywhere in a batch, at any z-chunk depth of any scale,
 *            after any sub-batch split, through every entry point, on every call, with one gradient or both, and for any view of the
 *            same voxels.  One writer per gradient voxel, no floating-point atomics.
 *   Reach    a window reads nothing beyond its radius at any scale; it is not a zero-padded 11-tap window.
 *   Accuracy measured per window against the float64 model: tests/msssim3k_model.py (EMU, ODD_EMU) and DESIGN.md section 27.
 *
 * Arguments, EINVAL / ENODEV rules, sub-batches, scratch (it does not depend on the window) and stream behaviour are those of the entry
 * without _win.  Additional EINVAL, checked after that entry's sample type, data range, pairs, scales and weights, before its other
 * pointers and before the context or any device is touched: a size outside the five, an unknown kind, a Gaussian sigma that is not
 * finite or not > 0.  _host without a device: ENODEV.
 *
 * Follow-up, not in this interface: a multi-scale map gradient.
 */
rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3f_win(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                const double* weights, double* valuesDevice, double* scaleMeansDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssim3f_win_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                       float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                       const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssim3f_win_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                     float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                     const double* weights, float* msssim, double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3f_win_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3F* params,
                                                     float dataRange, const rmgr_ssim_hip_Window* window, rmgr_uint32_t scales,
                                                     const double* weights, const double* scaleMeansDevice, const float* gradOutDevice,
                                                     const rmgr_ssim_hip_Grad3F* gradA, const rmgr_ssim_hip_Grad3F* gradB) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3h_win(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                rmgr_uint32_t scales, const double* weights, double* valuesDevice,
                                                double* scaleMeansDevice) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssim3h_win_device(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                       rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                       rmgr_uint32_t scales, const double* weights, float* msssim,
                                                       double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_compute_msssim3h_win_host(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                     rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                     rmgr_uint32_t scales, const double* weights, float* msssim,
                                                     double* scaleMeans) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_enqueue_msssim3h_win_grad(rmgr_ssim_hip_Context* ctx, rmgr_uint32_t count, const rmgr_ssim_hip_Params3H* params,
                                                     rmgr_uint32_t sampleType, float dataRange, const rmgr_ssim_hip_Window* window,
                                                     rmgr_uint32_t scales, const double* weights, const double* scaleMeansDevice,
                                                     const float* gradOutDevice, const rmgr_ssim_hip_Grad3H* gradA,
                                                     const rmgr_ssim_hip_Grad3H* gradB) RMGR_NOEXCEPT;

/*
 * Multi-GPU exchange without any other runtime: one process per GPU, images sharded by rank (no image
 * data crosses GPUs), every rank enqueues its shard into ITS slice of a zero-initialised device vector
 * of per-image fp64 sums, then all ranks call comm_allreduce_sums on the whole vector: one RCCL
 * all-reduce(sum, fp64) over xGMI.  Adding zeros is exact, so the result does not depend on the GPU
 * count.  This is the GPU-era form of the reference's per-thread partials + final loop
 * (src/ssim.cpp:902-926, :1094-1100).  librccl is loaded on first use ($RMGR_SSIM_HIP_RCCL_LIB, else the
 * copy already in the process or the system's); ENOSYS if it is absent.
 *   rank 0: comm_get_unique_id(id); ship the 128 bytes to the other ranks by any means (file, socket, MPI)
 *   all:    comm_init(ctx, id, rankCount, rank);  ...  comm_allreduce_sums(ctx, sumsDevice, count);
 *
 * Bounded failure.  Where the reference reports a failed worker as ECHILD (src/ssim.cpp:1094-1097), a rank that never
 * arrives is reported here as ETIMEDOUT after $RMGR_SSIM_HIP_COMM_TIMEOUT_S seconds (default 30): get_unique_id and
 * comm_init (library load, bootstrap, rendezvous), the enqueue inside comm_allreduce_sums, and every wait for a QUEUED
 * all-reduce -- rmgr_ssim_hip_synchronize(), comm_destroy and rmgr_ssim_hip_destroy on a context with all-reduces outstanding --
 * are bounded by it.  The deadline of a queued all-reduce runs from the moment its turn on the stream has come, not from the call:
 * kernels queued before or after it may take as long as they take (each all-reduce sits between two events; the wait polls them,
 * sleeping 50 us ... 1 ms between polls).  Past the deadline the communicator is aborted (ncclCommAbort), which releases the
 * kernel that waits for the missing peers; the wait for that kernel to leave is bounded by one more such interval.  A library
 * without ncclCommAbort cannot release it: ETIMEDOUT is returned and the stream is left as it is.  ncclCommDestroy of a BLOCKING
 * communicator ($RMGR_SSIM_HIP_COMM_BLOCKING=1) waits for the peers inside RCCL and is not bounded; the default (non-blocking)
 * communicator's teardown is.  After ETIMEDOUT the context is back in its single-GPU state -- it still computes, and
 * comm_init may be called again (tests/test_gpu_zz_rccl.py does both).  How: library load, ncclGetUniqueId and the
 * communicator's creation run on a helper thread the caller waits for with a timeout; the communicator is requested
 * non-blocking (ncclCommInitRankConfig, blocking = 0) and, if the deadline passes while its rendezvous is in progress,
 * aborted (ncclCommAbort) by the helper.  On the RCCL builds of this image (2.26.6 in the PyTorch wheel, 2.27.7 in
 * /opt/rocm) that call carries the rendezvous out before it returns, blocking = 0 notwithstanding (measured:
 * profiles/r04_final_rccl_selftest.txt), so what bounds comm_init there is the helper's timeout: the helper stays parked
 * inside RCCL and is abandoned (one idle thread; nothing it touches lives on the caller's stack).  Caveats of an abandoned helper: it is
 * still inside librccl when the process exits or this library is unloaded (exit from main is safe -- the thread is never joined and owns
 * its data --, dlclose() of this library while it exists is not); and while a FIRST use is still loading librccl on another thread,
 * comm_describe / comm_allreduce_sums / comm_destroy report "not loadable" / ENOSYS instead of waiting for that load.  Helpers never read
 * the environment: $RMGR_SSIM_HIP_RCCL_LIB, _COMM_DEBUG and _COMM_TIMEOUT_S are read on the calling thread of each entry point.
 * $RMGR_SSIM_HIP_COMM_BLOCKING=1 asks for a plain blocking communicator; $RMGR_SSIM_HIP_COMM_DEBUG=1 logs the helper's
 * steps on stderr.
 */
#define RMGR_SSIM_HIP_COMM_ID_BYTES 128
rmgr_int32_t rmgr_ssim_hip_comm_get_unique_id(unsigned char id[RMGR_SSIM_HIP_COMM_ID_BYTES]) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_comm_init(rmgr_ssim_hip_Context* ctx, const unsigned char id[RMGR_SSIM_HIP_COMM_ID_BYTES],
                                     rmgr_int32_t rankCount, rmgr_int32_t rank) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_comm_allreduce_sums(rmgr_ssim_hip_Context* ctx, double* sumsDevice, rmgr_uint32_t count) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_comm_destroy(rmgr_ssim_hip_Context* ctx) RMGR_NOEXCEPT;
/* Ranks RCCL itself counts in the context's communicator (ncclCommCount); 0 when it has none. */
rmgr_int32_t rmgr_ssim_hip_comm_rank_count(const rmgr_ssim_hip_Context* ctx, rmgr_int32_t* rankCount) RMGR_NOEXCEPT;
/* Which RCCL was loaded (version, path), whether non-blocking init is available, the deadline in force; static storage. */
const char* rmgr_ssim_hip_comm_describe(void) RMGR_NOEXCEPT;

/* Blocks until everything enqueued on the context's stream has finished. */
rmgr_int32_t rmgr_ssim_hip_synchronize(rmgr_ssim_hip_Context* ctx) RMGR_NOEXCEPT;

/* Device memory for hosts that have no HIP runtime of their own. */
rmgr_int32_t rmgr_ssim_hip_malloc(rmgr_ssim_hip_Context* ctx, void** devicePtr, size_t size) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_free(rmgr_ssim_hip_Context* ctx, void* devicePtr) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_memcpy_h2d(rmgr_ssim_hip_Context* ctx, void* devicePtr, const void* hostPtr, size_t size) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_memcpy_d2h(rmgr_ssim_hip_Context* ctx, void* hostPtr, const void* devicePtr, size_t size) RMGR_NOEXCEPT;

/*
 * Kernel timing with HIP events on the context's stream.  While enabled, every launch of the
 * main SSIM kernel is bracketed by an event pair; get_profile() (after a synchronize) returns
 * how many launches were timed and their summed duration in milliseconds, then resets.
 * "Launch" means kernel launch, not API call: a host-pointer call that asks for a map is pipelined
 * over row bands (one kernel launch per band) and therefore counts as several launches.
 */
rmgr_int32_t rmgr_ssim_hip_set_profiling(rmgr_ssim_hip_Context* ctx, rmgr_int32_t enabled) RMGR_NOEXCEPT;
rmgr_int32_t rmgr_ssim_hip_get_profile(rmgr_ssim_hip_Context* ctx, rmgr_uint64_t* launches, double* kernelMs) RMGR_NOEXCEPT;
/* The shader clock the profiled launches really ran at (round 6).  While profiling is enabled, the first workgroups of every strip-kernel launch -- one per XCD: the
 * dispatcher deals consecutive workgroups to the XCDs round robin -- read s_memtime (one tick per shader cycle) and s_memrealtime (the constant reference clock,
 * hipDeviceAttributeWallClockRate: 100 MHz) when they start and when they end and add the differences to per-XCD device counters; this call (it waits for the stream)
 * returns *shaderMHz = the mean over the XCDs of reference rate x cycles / ticks, *slowestXcdMHz = the lowest XCD's (a launch ends when its slowest XCD does) and how many
 * launches contributed (0 and 0.0 if none), then clears the counters.  Boxes of one pool differ in the clock they sustain under THIS kernel's load by more than they
 * differ under a pure FMA stream; lane-operations per CYCLE are what a kernel change changes.  Any pointer may be NULL. */
rmgr_int32_t rmgr_ssim_hip_get_profile_clock(rmgr_ssim_hip_Context* ctx, double* shaderMHz, double* slowestXcdMHz, rmgr_uint64_t* launches) RMGR_NOEXCEPT;

/*
 * What the vector ALUs of the context's device sustain RIGHT NOW at a forced occupancy (profiling aid; no reference counterpart; not on
 * the SSIM path).  A pure packed-fp32 instruction stream runs with its register footprint padded so that the hardware cannot place more
 * than wavesPerSimd (1, 2, 3, 4 or 8) wavefronts on a SIMD, on a grid of exactly the device's capacity at that occupancy; streamKind 0:
 * independent v_pk_fma_f32 (the issue peak at that occupancy), 1: two interleaved dependent chains of six (the blur's row sums).  Twenty untimed
 * launches (~40 ms: the clock leaves its idle state), then `launches` (1 ... 64) timed ones of about 2 ms each between HIP events on the context's stream, all
 * enqueued back to back and waited for once (a host-side wait between launches is an idle gap after which the clock ramps again); three such bursts, the best
 * one counts (about one burst in four runs in a degraded mode -- same clock, the rate of one wave fewer per SIMD: profiles/r06_probe_bimodal.txt); *teraLaneOps
 * receives the best burst's MEDIAN launch's rate in 10^12 lane-operations per second (128 per packed instruction and wavefront).  The strip kernels are
 * fp32-VALU bound and run at two (modes 0, 1, 3) or three (modes 2, 4) wavefronts per SIMD: bench.py divides their lane-operations per
 * second by this figure, measured in the same process right before and right after the timed steps, instead of by a constant measured on
 * another box.  shaderMHz / slowestXcdMHz (may be NULL): the shader clock the timed launches really ran at -- mean over the XCDs, and the slowest XCD's --
 * measured on the device as rmgr_ssim_hip_get_profile_clock measures the strip kernels'.  Blocking.  EINVAL for any other occupancy or stream kind.
 */
rmgr_int32_t rmgr_ssim_hip_probe_valu(rmgr_ssim_hip_Context* ctx, rmgr_int32_t wavesPerSimd, rmgr_int32_t streamKind, rmgr_int32_t launches,
                                      double* teraLaneOps, double* shaderMHz, double* slowestXcdMHz) RMGR_NOEXCEPT;

/*
 * The synthetic test pattern the benchmark and the self-tests run on (no reference counterpart: the reference's
 * tests read image files), generated in device memory, asynchronously on the context's stream:
 *   r = splitmix64(seed ^ ((y << 32) | x));  g = ((3x + 5y) >> 2) & 255;  A = (3g + (r & 255)) >> 2;
 *   B = clamp(A + ((r >> 8) % 33) - 16, 0, 255)          planar, one byte per pixel, rows stride bytes apart.
 * Known answers: seed 0x5EED gives A[0][0..3] = 45, 59, 51, 6 and B[0][0..3] = 51, 58, 48, 5.
 */
rmgr_int32_t rmgr_ssim_hip_synth_pair_device(rmgr_ssim_hip_Context* ctx, rmgr_uint8_t* imgA, ptrdiff_t strideA, rmgr_uint8_t* imgB, ptrdiff_t strideB,
                                             rmgr_uint32_t width, rmgr_uint32_t height, rmgr_uint64_t seed) RMGR_NOEXCEPT;

/* Human-readable description of the device and build ("gfx950 ... CUs ..."); static storage. */
const char* rmgr_ssim_hip_describe(rmgr_ssim_hip_Context* ctx) RMGR_NOEXCEPT;

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RMGR_SSIM_HIP_H */
