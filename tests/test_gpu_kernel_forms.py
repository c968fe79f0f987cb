"""GPU: every kernel form, in every arithmetic mode, against a per-pixel reference of that mode.

The bit-exact modes meet the oracle bit for bit on random layouts and extreme shapes (test_gpu_fuzz.py, test_gpu_extreme.py);
the other modes were held to their bounds on dense images only.  Here each mode meets its reference where the kernels take
their less common forms:

  * the 64-bit one-column form, ssim_strip1_kernel<MODE, MAP, WIDE=true>.  It runs for a pair that fits_strip2() rejects (a
    pixel or map step of magnitude 2^21 or more, e.g. a slice taken across the slices of a volume) and for a whole batch that
    holds one such pair.  All five modes, with and without a map;
  * both sides of fits_strip2(): the same pixels at step 2^21 - 1 (the 32-bit forms) and at step 2^21 (the 64-bit form);
  * random image and map layouts, extreme shapes, the division's corner statistics and the banded host-pointer call, in the
    modes that are not bit-exact.

References and bounds are the ones tests/test_gpu_modes.py asserts on dense images:
  MODE_EXACT / MODE_UNFUSED    oracle.ssim_f32(fused=True / False)  every pixel bit-identical, global value <= 1 ulp
  MODE_FAST / MODE_SEPARABLE   tests/tools/fast_mode_model.py       every pixel <= 3 ulp, global <= 3.3e-7 from float32(model mean)
  MODE_DOUBLE                  oracle.ssim_naive_f64                every pixel <= 1e-7, global <= 6e-8 + 1e-9
In every mode the map and the value are also bit-identical to the same mode's dense call with default tuning: the kernels of
a mode agree bit for bit across variants, strip heights and forms.  Every map buffer starts filled with a sentinel, and no
element outside the map's own elements may change.
"""
import os
import sys

import numpy as np
import pytest

import ssim_amd
from conftest import f32_hex, ulp_diff
from test_gpu_extreme import EXTREME_SHAPES
from test_gpu_fuzz import make_layout
from test_gpu_parity import assert_same_map
from test_gpu_pipeline import hostile_pairs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import fast_mode_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT, FAST, DOUBLE, UNFUSED, SEPARABLE = (ssim_amd.MODE_EXACT, ssim_amd.MODE_FAST, ssim_amd.MODE_DOUBLE,
                                           ssim_amd.MODE_UNFUSED, ssim_amd.MODE_SEPARABLE)
MODES = (EXACT, UNFUSED, FAST, SEPARABLE, DOUBLE)
NAME = {EXACT: "EXACT", UNFUSED: "UNFUSED", FAST: "FAST", SEPARABLE: "SEPARABLE", DOUBLE: "DOUBLE"}
# (per-pixel bound, global bound).  Float32 ulps for the pixels of the fp32 modes and for the global value of the bit-exact
# modes; absolute differences otherwise.
BOUND = {EXACT: (0, 1), UNFUSED: (0, 1), FAST: (3, 3.3e-7), SEPARABLE: (3, 3.3e-7), DOUBLE: (1e-7, 6e-8 + 1e-9)}
EDGE = 1 << 21        # fits_strip2(): a pixel or map step of this magnitude or more takes the 64-bit form
SENTINEL = -3.0


def threads(oracle):
    return min(oracle.oracle_lib().oracle_max_threads(), 16)


def reference(oracle, mode, a, b):
    """(per-pixel reference map, reference global value) of `mode` on the dense pair (a, b)."""
    if mode in (EXACT, UNFUSED):
        v, _, m = oracle.ssim_f32(a, b, want_map=True, fused=(mode == EXACT), threads=threads(oracle))
        return m, v
    if mode == DOUBLE:
        v, _, m = oracle.ssim_naive_f64(a, b, want_map=True, threads=threads(oracle))
        return m, v
    m = (model.mode_fast if mode == FAST else model.mode_separable)(a, b)
    return m, np.float32(m.astype(np.float64).sum() / np.float64(m.size))


def check(mode, got_map, got_v, ref_map, ref_v, worst, form):
    """Asserts `mode`'s bounds on one result (got_map None: the global value only) and keeps the worst errors per (mode, form)."""
    px = 0
    if mode == DOUBLE:
        if got_map is not None:
            px = float(np.abs(got_map.astype(np.float64) - ref_map).max())
        g = abs(float(got_v) - float(ref_v))
    else:
        if got_map is not None:
            px = int(ulp_diff(got_map, ref_map).max())
        g = int(ulp_diff(got_v, ref_v)) if mode in (EXACT, UNFUSED) else abs(float(got_v) - float(ref_v))
    key = (MODES.index(mode), form)
    wp, wg = worst.get(key, (0, 0))
    worst[key] = (max(wp, px), max(wg, g))
    assert px <= BOUND[mode][0], (NAME[mode], form, "per-pixel error", px)
    assert g <= BOUND[mode][1], (NAME[mode], form, "global error", g, float(got_v), float(ref_v))


def report(title, worst):
    print("\n%s: worst error per mode and form (bound)" % title)
    for (i, form), (px, g) in sorted(worst.items()):
        mode = MODES[i]
        pxs = "%.3g (%.3g)" % (px, BOUND[mode][0]) if mode == DOUBLE else "%d ulp (%d ulp)" % (px, BOUND[mode][0])
        gs = "%d ulp (%d ulp)" % (g, BOUND[mode][1]) if mode in (EXACT, UNFUSED) else "%.3g (%.3g)" % (g, BOUND[mode][1])
        print("  %-9s %-34s per pixel %-22s global %s" % (NAME[mode], form, pxs, gs))


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def noisy_pair(rng, h, w, spread=30):
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return a, np.clip(a.astype(np.int32) + rng.integers(-spread, spread + 1, (h, w)), 0, 255).astype(np.uint8)


# ---- image and map layouts ----------------------------------------------------------------------------------------------
def column_buffer(img, step):
    """The bytes of a plane whose column x starts at byte x * step, its rows one byte apart (a slice taken across the slices of
    a volume); every other byte holds a filler."""
    h, w = img.shape
    buf = np.full((w - 1) * step + h, 0xA5, np.uint8)
    buf[np.arange(h)[:, None] + np.arange(w)[None, :] * step] = img
    return buf


def column_view(dev, img, step, flip_x, flip_y):
    """A column buffer on the device read mirrored (step -step) and / or bottom-up (stride -1): the (pointer to pixel (0,0),
    step, stride) triple and the plane it addresses."""
    h, w = img.shape
    off = ((w - 1) * step if flip_x else 0) + (h - 1 if flip_y else 0)
    seen = np.ascontiguousarray(img[::-1 if flip_y else 1, ::-1 if flip_x else 1])
    return (dev.ptr + off, -step if flip_x else step, -1 if flip_y else 1), seen


def dense_map(h, w, bottom_up=False, pad=8):
    """Map layout (floats in the buffer, offset of element (0,0), step, stride, index of every element): W x H, rows
    top-down or bottom-up, `pad` floats of sentinel before and after."""
    off, stride = (pad + (h - 1) * w, -w) if bottom_up else (pad, w)
    return h * w + 2 * pad, off, 1, stride, off + np.arange(h)[:, None] * stride + np.arange(w)[None, :]


def random_map_layout(rng, h, w):
    """Map layout with a step of 1..3 floats, padded rows, rows and / or columns in reverse order."""
    mstep = int(rng.integers(1, 4))
    mrow = w * mstep + int(rng.integers(0, 5))
    flip_y, flip_x = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    off = 2 + ((h - 1) * mrow if flip_y else 0) + ((w - 1) * mstep if flip_x else 0)
    step, stride = (-mstep if flip_x else mstep), (-mrow if flip_y else mrow)
    return h * mrow + 8, off, step, stride, off + np.arange(h)[:, None] * stride + np.arange(w)[None, :] * step


def random_images(ctx, rng, a, b, keep):
    """a and b uploaded in random layouts (test_gpu_fuzz.make_layout): their (pointer, step, stride) triples."""
    out = []
    for img in (a, b):
        buf, off, step, stride = make_layout(rng, img)
        d = ctx.upload(buf)
        keep.append(d)
        out.append((d.ptr + off, step, stride))
    return out


def read_map(dm, mlay):
    """The map elements of a sentinel-filled device buffer in image orientation; asserts that nothing else was written."""
    n, _, _, _, idx = mlay
    got = dm.download(np.float32, (n,))
    m = got[idx]
    got[idx] = SENTINEL
    assert np.all(got == SENTINEL), "elements outside the map changed"
    return m


def device_call(ctx, w, h, ia, ib, mlay=None):
    """rmgr_ssim_hip_compute_ssim_device on image triples ia, ib; with a map laid out as `mlay` in a sentinel-filled buffer."""
    if mlay is None:
        return ctx.compute_device(ssim_amd.make_params(w, h, *(ia + ib))), None
    dm = ctx.upload(np.full(mlay[0], SENTINEL, np.float32))
    try:
        v = ctx.compute_device(ssim_amd.make_params(w, h, *(ia + ib), map_ptr=dm.ptr + 4 * mlay[1], map_step=mlay[2], map_stride=mlay[3]))
        return v, read_map(dm, mlay)
    finally:
        dm.free()


def batch_call(ctx, w, h, images, mlays=None):
    """One rmgr_ssim_hip_enqueue_batch over `images` (a list of (ia, ib) triples) with a map per pair laid out as mlays[i], or
    none: the per-image fp64 sums and the maps."""
    n = len(images)
    bufs, params = [], []
    try:
        for i, (ia, ib) in enumerate(images):
            if mlays is None:
                params.append(ssim_amd.make_params(w, h, *(ia + ib)))
                continue
            dm = ctx.upload(np.full(mlays[i][0], SENTINEL, np.float32))
            bufs.append(dm)
            params.append(ssim_amd.make_params(w, h, *(ia + ib), map_ptr=dm.ptr + 4 * mlays[i][1], map_step=mlays[i][2], map_stride=mlays[i][3]))
        sums = ctx.upload(np.full(n, np.nan))
        bufs.append(sums)
        ctx.enqueue_batch((ssim_amd.Params * n)(*params), n, sums.ptr)
        ctx.synchronize()
        s = sums.download(np.float64, (n,))
        maps = None if mlays is None else [read_map(bufs[i], mlays[i]) for i in range(n)]
    finally:
        for d in bufs:
            d.free()
    return s, maps


def finalize1(s, w, h):
    return ssim_amd.finalize(np.array([s]), w, h)[0]


# ---- the 64-bit one-column form -----------------------------------------------------------------------------------------
def test_far_apart_pixels_take_the_64_bit_form_in_every_mode(gpu_ctx, oracle):
    """Pixels 2^21 + 3 bytes apart, rows one byte apart, and the same buffers read with step -(2^21 + 3) (A mirrored, B mirrored
    and bottom-up): fits_strip2() is false, so every launch runs ssim_strip1_kernel<MODE, MAP, WIDE=true>.  150 x 40 pixels:
    two full 64-column strips and a ragged one, five strip rows of 8 (and the default strips).  Dense, bottom-up and no map;
    single calls, and batches of the pair alone and mixed with ordinary pairs (the whole launch then takes the 64-bit form)."""
    rng = np.random.default_rng(0xFA2A)
    h, w, step = 40, 150, EDGE + 3
    a, b = noisy_pair(rng, h, w)
    ordinary = hostile_pairs(rng, w, h, 3)
    maps = (("dense map", dense_map(h, w)), ("bottom-up map", dense_map(h, w, bottom_up=True)), ("no map", None))
    flips = (("step +(2^21+3)", (False, False, False, False)), ("step -(2^21+3)", (True, False, True, True)))
    unit = dense_map(h, w)
    worst = {}
    keep = []
    try:
        fa, fb = gpu_ctx.upload(column_buffer(a, step)), gpu_ctx.upload(column_buffer(b, step))      # ~315 MB each
        keep += [fa, fb]
        da, db = gpu_ctx.upload(a), gpu_ctx.upload(b)
        keep += [da, db]
        plain = []
        for x, y in ordinary:
            dx, dy = gpu_ctx.upload(x), gpu_ctx.upload(y)
            keep += [dx, dy]
            plain.append(((dx.ptr, 1, w), (dy.ptr, 1, w)))
        for mode in MODES:
            gpu_ctx.set_mode(mode)
            for form, (ax, ay, bx, by) in flips:
                ia, sa = column_view(fa, a, step, ax, ay)
                ib, sb = column_view(fb, b, step, bx, by)
                ref_m, ref_v = reference(oracle, mode, sa, sb)
                gpu_ctx.set_tuning(0, 0)
                dv, dm = gpu_ctx.ssim_planes(sa, sb, want_map=True)
                check(mode, dm, dv, ref_m, ref_v, worst, "dense images")
                for rows in (8, 0):
                    gpu_ctx.set_tuning(rows, 0)
                    for mname, mlay in maps:
                        v, m = device_call(gpu_ctx, w, h, ia, ib, mlay)
                        what = "%s, %s, %d-row strips, %s" % (NAME[mode], form, rows, mname)
                        assert f32_hex(v) == f32_hex(dv), what
                        if m is not None:
                            assert_same_map(m, dm, what)
                        check(mode, m, v, ref_m, ref_v, worst, "64-bit, " + mname)

            # batches: the far-apart pair alone, with and without a map, equals the dense pair's sum
            gpu_ctx.set_tuning(0, 0)
            far = (column_view(fa, a, step, False, False)[0], column_view(fb, b, step, False, False)[0])
            s_dense, m_dense = batch_call(gpu_ctx, w, h, [((da.ptr, 1, w), (db.ptr, 1, w))], [unit])
            s_far, _ = batch_call(gpu_ctx, w, h, [far])
            s_far_m, m_far = batch_call(gpu_ctx, w, h, [far], [unit])
            assert np.array_equal(bits64(s_far), bits64(s_dense)) and np.array_equal(bits64(s_far_m), bits64(s_dense)), (NAME[mode], s_far, s_far_m, s_dense)
            assert_same_map(m_far[0], m_dense[0], NAME[mode] + ", far-apart pair in a batch")
            # ... and mixed with ordinary pairs of the same size: every sum and map as in the batches without it
            s_plain, m_plain = batch_call(gpu_ctx, w, h, plain, [unit] * len(plain))
            s_plain_n, _ = batch_call(gpu_ctx, w, h, plain)
            assert np.array_equal(bits64(s_plain_n), bits64(s_plain)), NAME[mode]
            for i, (x, y) in enumerate(ordinary):
                ref_m, ref_v = reference(oracle, mode, x, y)
                check(mode, m_plain[i], finalize1(s_plain[i], w, h), ref_m, ref_v, worst, "ordinary pairs, batch")
            mixed = [plain[0], far] + plain[1:]
            for with_map in (False, True):
                s_mix, m_mix = batch_call(gpu_ctx, w, h, mixed, [unit] * len(mixed) if with_map else None)
                what = "%s, mixed batch, %s" % (NAME[mode], "maps" if with_map else "no maps")
                assert np.array_equal(bits64(s_mix[1:2]), bits64(s_far)), (what, s_mix[1], s_far[0])
                assert np.array_equal(bits64(np.delete(s_mix, 1)), bits64(s_plain)), (what, np.delete(s_mix, 1) - s_plain)
                if with_map:
                    assert_same_map(m_mix[1], m_far[0], what + ", far-apart pair")
                    for i in range(len(plain)):
                        assert_same_map(m_mix[i + 1 if i else 0], m_plain[i], what + ", ordinary pair %d" % i)
    finally:
        gpu_ctx.set_tuning(0, 0)
        gpu_ctx.set_mode(EXACT)
        for d in keep:
            d.free()
    report("far-apart pixels (150 x 40, step +-(2^21 + 3))", worst)


def test_both_sides_of_the_32_bit_limit(gpu_ctx, oracle):
    """fits_strip2() accepts steps of magnitude up to 2^21 - 1.  The same pixels at step 2^21 - 1 run the 32-bit forms (tuning
    variant 0 with 8-row strips: the two-column kernel, with early row sums in the bit-exact modes; 1: the one-column kernel;
    2: the two-column kernel), at step 2^21 the 64-bit one-column form whatever the variant asks.  Both signs of the step.
    Every launch is also repeated without a map, and with the map's own step at the edge: 2^21 - 1 floats across 150 columns
    (a 1.25 GB buffer, mirrored with the images)."""
    rng = np.random.default_rng(0xED6E)
    h, w = 40, 150
    a, b = noisy_pair(rng, h, w, 60)
    mstep = EDGE - 1
    nfar = (w - 1) * mstep + h
    unit = dense_map(h, w)
    dense, worst, seen_forms = {}, {}, 0
    keep = []
    try:
        far_map = gpu_ctx.upload(np.full(nfar, SENTINEL, np.float32))
        keep.append(far_map)
        for step in (EDGE - 1, EDGE):
            fa, fb = gpu_ctx.upload(column_buffer(a, step)), gpu_ctx.upload(column_buffer(b, step))
            keep += [fa, fb]
            for flip in (False, True):
                ia, sa = column_view(fa, a, step, flip, False)
                ib, sb = column_view(fb, b, step, flip, flip)
                form = "%s2^21%s" % ("-" if flip else "+", " - 1" if step == EDGE - 1 else "")
                for mode in MODES:
                    gpu_ctx.set_mode(mode)
                    if (flip, mode) not in dense:
                        gpu_ctx.set_tuning(0, 0)
                        dv, dm = gpu_ctx.ssim_planes(sa, sb, want_map=True)
                        dense[(flip, mode)] = (dv, dm) + reference(oracle, mode, sa, sb)
                    dv, dm, ref_m, ref_v = dense[(flip, mode)]
                    for variant in ((0,) if mode == DOUBLE else (0, 1, 2)):
                        gpu_ctx.set_tuning(8, variant)
                        what = "%s, step %s, variant %d" % (NAME[mode], form, variant)
                        v, m = device_call(gpu_ctx, w, h, ia, ib, unit)
                        assert f32_hex(v) == f32_hex(dv), what
                        assert_same_map(m, dm, what)
                        check(mode, m, v, ref_m, ref_v, worst, "step " + form)
                        v, _ = device_call(gpu_ctx, w, h, ia, ib)
                        assert f32_hex(v) == f32_hex(dv), what + ", no map"
                        # the map step at the edge as well
                        p = ssim_amd.make_params(w, h, *(ia + ib), map_ptr=far_map.ptr + (4 * (w - 1) * mstep if flip else 0),
                                                 map_step=-mstep if flip else mstep, map_stride=1)
                        v = gpu_ctx.compute_device(p)
                        cols = [gpu_ctx.download(far_map.ptr + 4 * ((w - 1 - x) if flip else x) * mstep, np.float32, (h,)) for x in range(w)]
                        m = np.ascontiguousarray(np.stack(cols, axis=1))
                        assert f32_hex(v) == f32_hex(dv), what + ", map step at the edge"
                        assert_same_map(m, dm, what + ", map step at the edge")
                        check(mode, m, v, ref_m, ref_v, worst, "step " + form + ", map step edge")
                        seen_forms += 1
            fa.free()
            fb.free()
        got = far_map.download(np.float32, (nfar,))
        far_map.free()
        got[(np.arange(h)[:, None] + np.arange(w)[None, :] * mstep).ravel()] = SENTINEL
        assert np.all(got == SENTINEL), "elements outside the far-apart map changed"
        del got
    finally:
        gpu_ctx.set_tuning(0, 0)
        gpu_ctx.set_mode(EXACT)
        for d in keep:
            d.free()
    assert seen_forms == 2 * 2 * 13
    report("both sides of fits_strip2() (150 x 40)", worst)


# ---- random layouts, extreme shapes, corner statistics, host pointers in the modes that are not bit-exact ----------------
@pytest.mark.parametrize("mode", [FAST, SEPARABLE, DOUBLE])
def test_random_layouts_against_the_reference(gpu_ctx, oracle, mode):
    """test_gpu_fuzz.test_random_layouts_bit_exact in the other modes: any pixel step 1..4 with padding, flips, column-major
    storage, map steps 1..3 with padding and flips, tuning variants 0..2 and strip heights 0, 1, 3, 16, 50.  Then one batch of
    nine pairs of one size, each in its own layouts: every per-image sum equals the pair's single call bit for bit."""
    rng = np.random.default_rng(20261016 + mode)
    worst = {}
    gpu_ctx.set_mode(mode)
    keep = []
    try:
        for case in range(40):
            h, w = int(rng.integers(1, 201)), int(rng.integers(1, 301))
            a, b = noisy_pair(rng, h, w)
            if rng.integers(0, 3) == 0:
                b = rng.integers(0, 256, (h, w), dtype=np.uint8)
            variant, rows = int(rng.integers(0, 3)), int(rng.choice([0, 1, 3, 16, 50]))
            ref_m, ref_v = reference(oracle, mode, a, b)
            gpu_ctx.set_tuning(0, 0)
            dv, dm = gpu_ctx.ssim_planes(a, b, want_map=True)
            check(mode, dm, dv, ref_m, ref_v, worst, "dense")
            try:
                ia, ib = random_images(gpu_ctx, rng, a, b, keep)
                gpu_ctx.set_tuning(rows, variant)
                v, m = device_call(gpu_ctx, w, h, ia, ib, random_map_layout(rng, h, w))
            finally:
                for d in keep:
                    d.free()
                keep = []
            what = "%s case %d: %d x %d, variant %d, rows %d, A %s, B %s" % (NAME[mode], case, w, h, variant, rows, ia[1:], ib[1:])
            assert f32_hex(v) == f32_hex(dv), what
            assert_same_map(m, dm, what)
            check(mode, m, v, ref_m, ref_v, worst, "random layouts")

        h, w = int(rng.integers(9, 201)), int(rng.integers(65, 301))
        pairs = hostile_pairs(rng, w, h, 9)
        variant, rows = int(rng.integers(0, 3)), int(rng.choice([0, 1, 3, 16, 50]))
        images = [random_images(gpu_ctx, rng, x, y, keep) for x, y in pairs]
        mlays = [random_map_layout(rng, h, w) for _ in pairs]
        gpu_ctx.set_tuning(rows, variant)
        sums, maps = batch_call(gpu_ctx, w, h, images, mlays)
        gpu_ctx.set_tuning(0, 0)
        for i, (x, y) in enumerate(pairs):
            one, _ = batch_call(gpu_ctx, w, h, [images[i]])
            v = gpu_ctx.compute_device(ssim_amd.make_params(w, h, *(images[i][0] + images[i][1])))
            what = "%s batch of 9 (%d x %d, variant %d, rows %d), pair %d" % (NAME[mode], w, h, variant, rows, i)
            assert bits64(sums[i:i + 1])[0] == bits64(one)[0], (what, sums[i], one[0])
            assert f32_hex(finalize1(sums[i], w, h)) == f32_hex(v), what
            dv, dm = gpu_ctx.ssim_planes(x, y, want_map=True)
            assert_same_map(maps[i], dm, what)
            ref_m, ref_v = reference(oracle, mode, x, y)
            check(mode, maps[i], v, ref_m, ref_v, worst, "batch, random layouts")
    finally:
        gpu_ctx.set_tuning(0, 0)
        gpu_ctx.set_mode(EXACT)
        for d in keep:
            d.free()
    report("random layouts", worst)


@pytest.mark.parametrize("w,h", EXTREME_SHAPES)
@pytest.mark.parametrize("mode", [FAST, SEPARABLE, DOUBLE])
def test_very_wide_and_very_tall_images_against_the_reference(gpu_ctx, oracle, mode, w, h):
    """The shapes of test_gpu_extreme.test_very_wide_and_very_tall_images_bit_exact, every pixel against the mode's reference,
    with the default tuning and with the one-column kernel on 16-row strips (the same bits)."""
    rng = np.random.default_rng(w * 31 + h)
    a, b = noisy_pair(rng, h, w, 40)
    gpu_ctx.set_mode(mode)
    try:
        gpu_ctx.set_tuning(0, 0)
        v, m = gpu_ctx.ssim_planes(a, b, want_map=True)
        gpu_ctx.set_tuning(16, 1)
        v1, m1 = gpu_ctx.ssim_planes(a, b, want_map=True)
    finally:
        gpu_ctx.set_tuning(0, 0)
        gpu_ctx.set_mode(EXACT)
    assert f32_hex(v1) == f32_hex(v)
    assert_same_map(m1, m, "%s %d x %d, one-column kernel" % (NAME[mode], w, h))
    worst = {}
    ref_m, ref_v = reference(oracle, mode, a, b)
    check(mode, m, v, ref_m, ref_v, worst, "%d x %d" % (w, h))
    report("extreme shapes", worst)


def test_double_mode_on_the_division_corners(gpu_ctx, oracle):
    """MODE_DOUBLE on the images of test_gpu_fuzz.test_division_corner_statistics_bit_exact -- anti-correlated textures whose
    covariance sweeps 2 sAB + c2 through zero, flat, saturated and checkerboard images -- and on the flat / saturated stress
    images of fast_mode_model.adversarial_pairs(): every pixel against the naive double reference."""
    rng = np.random.default_rng(4242)
    h, w = 200, 640
    xx = np.arange(w)[None, :].repeat(h, 0)
    cases = []
    for kk in (1.0, 0.5, 2.0, 1.0):
        amp = xx / w * (12.0 / np.sqrt(kk))
        t = rng.choice([-1.0, 1.0], (h, w))
        base = int(rng.integers(60, 196))
        cases.append(("sweeps", np.clip(np.rint(base + amp * t), 0, 255).astype(np.uint8), np.clip(np.rint(base - kk * amp * t), 0, 255).astype(np.uint8)))
    flat = "flat, saturated, checkerboard"
    cases += [(flat, np.zeros((40, 300), np.uint8), np.full((40, 300), 255, np.uint8)),
              (flat, np.full((40, 300), 255, np.uint8), np.full((40, 300), 255, np.uint8)),
              (flat, rng.choice([0, 255], (90, 400)).astype(np.uint8), rng.choice([0, 255], (90, 400)).astype(np.uint8)),
              (flat, (np.indices((64, 256)).sum(0) % 2 * 255).astype(np.uint8), (255 - np.indices((64, 256)).sum(0) % 2 * 255).astype(np.uint8))]
    cases += [("adversarial_pairs()", a, b) for _, a, b in model.adversarial_pairs()]
    worst = {}
    seen_small = seen_neg = 0
    gpu_ctx.set_mode(DOUBLE)
    try:
        for group, a, b in cases:
            v, m = gpu_ctx.ssim_planes(a, b, want_map=True)
            ref_m, ref_v = reference(oracle, DOUBLE, a, b)
            check(DOUBLE, m, v, ref_m, ref_v, worst, group)
            if group == "sweeps":
                seen_small += int((np.abs(ref_m) < 1e-3).sum())
                seen_neg += int((ref_m < 0).sum())
    finally:
        gpu_ctx.set_mode(EXACT)
    assert seen_small > 100 and seen_neg > 1000, (seen_small, seen_neg)      # the sweeps really crossed zero
    report("MODE_DOUBLE on corner statistics", worst)


@pytest.mark.parametrize("mode", [FAST, SEPARABLE, DOUBLE])
def test_banded_host_call_equals_the_device_call(gpu_ctx, oracle, mode):
    """rmgr_ssim_hip_compute_ssim_host on a context in the mode: large enough for the banded pipeline with a map (3000 x 1237),
    dense map, then bottom-up images with a bottom-up, padded map (the CPU-scatter path), then no map (one launch).  Value and
    every map pixel bit-identical to the device call."""
    w, h = 3000, 1237
    a, b = oracle.synth_pair(w, h, 0x5EED)
    af, bf = np.ascontiguousarray(a[::-1]), np.ascontiguousarray(b[::-1])
    gpu_ctx.set_mode(mode)
    try:
        v_dev, m_dev = gpu_ctx.ssim_planes(a, b, want_map=True)
        m = np.full((h, w), SENTINEL, np.float32)
        v = gpu_ctx.compute_host(ssim_amd.make_params(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w, m.ctypes.data, 1, w))
        assert f32_hex(v) == f32_hex(v_dev)
        assert_same_map(m, m_dev, NAME[mode] + ", host call, dense map")
        pad = np.full((h, w + 5), SENTINEL, np.float32)
        v2 = gpu_ctx.compute_host(ssim_amd.make_params(w, h, af.ctypes.data + (h - 1) * w, 1, -w, bf.ctypes.data + (h - 1) * w, 1, -w,
                                                       pad.ctypes.data + 4 * (h - 1) * (w + 5), 1, -(w + 5)))
        assert f32_hex(v2) == f32_hex(v_dev)
        assert_same_map(np.ascontiguousarray(pad[::-1, :w]), m_dev, NAME[mode] + ", host call, bottom-up")
        assert np.all(pad[:, w:] == SENTINEL)
        v3 = gpu_ctx.compute_host(ssim_amd.make_params(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w))
        assert f32_hex(v3) == f32_hex(v_dev)
    finally:
        gpu_ctx.set_mode(EXACT)
    print("\n%s host calls, 3000 x 1237: value and %d map pixels bit-identical to the device call (bound: bit-identical)" % (NAME[mode], m.size))
