"""GPU: SSIM of float16 / bfloat16 volumes under a caller-chosen window, its gradient and the gradient of its map
(rmgr_ssim_hip_*_ssim3h_win*; ssim3hk_kernels.hip for 3, 5, 7 and 9 taps, ssim3h_kernels.hip with the window's taps for 11) against the
float32 _win entries, BIT FOR BIT.  Sizes are W x H x D; arrays are (D, H, W); 16-bit samples travel as uint16 bit patterns.

The contract (include/rmgr/ssim-hip.h): value, map and fp64 sums have the bits rmgr_ssim_hip_enqueue_ssim3f_win gives on the widened
volumes under the same window; a gradient voxel is the float32 value of _enqueue_ssim3f_win_grad / _ssim3f_win_map_grad rounded once, to
nearest-even, into the inputs' encoding.  So every comparison here runs the float32 _win entry in the same test on
halfmodel.widen(samples) and compares bits -- gradients against halfmodel.round_to(float32 gradient) -- and no tolerance is new; NaN is
compared as NaN.  No float64 model runs here: tests/test_gpu_ssim3k.py holds the float32 windowed path to tests/ssim3k_model.py, and bit
equality carries that over.

Windows: the seven of ssimk_model.WINDOWS -- every radius kernel, and the 11-tap route with foreign taps.  Shapes, the smallest at which
a tile, cell, chunk or window edge can go wrong: 1x1x1; 3x5x2; 5x3x40; 17x17x9; 33x20x13; and 17x17x131 inside a launch of enough
volumes that tests/ssim3k_plan.py, at the device's CU count, gives chunks of at least 16 slices (asserted, never skipped).

The helpers are those of tests/test_gpu_ssim3h.py: all outputs of a call live in ONE buffer each with sentinel gaps (Arena), asserted
untouched after every call; after a return code that is neither success nor EINVAL the module starts nothing more on the GPU (the shared
_device_error).  The module prints its wall time and its peak device memory when it ends.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import halfmodel as HM
import ssim3h_inputs as IN
import ssim3k_plan as PK
import ssimk_model as K2
import ssim_amd
from conftest import ROOT
from test_gpu_ssim3h import Arena, Device, GAP, LAYOUTS, MAX16, NAN16, SENT, call, same64, widened
from test_gpu_ssimk import _device_error

pytestmark = pytest.mark.gpu

ENC = pytest.mark.parametrize("enc", HM.ENCODINGS)
WINDOWS = K2.WINDOWS
WINDOW_IDS = [K2.name_of(w) for w in WINDOWS]
WIN = pytest.mark.parametrize("window", WINDOWS, ids=WINDOW_IDS)
ONE_PER_RADIUS = [(3, 0.0, "uniform"), (5, 0.8, "gaussian"), (7, 0.0, "uniform"), (9, 1.5, "gaussian"), (11, 2.0, "gaussian")]
RADIUS = pytest.mark.parametrize("window", ONE_PER_RADIUS, ids=[K2.name_of(w) for w in ONE_PER_RADIUS])
SHAPES = [(1, 1, 1), (3, 5, 2), (5, 3, 40), (17, 17, 9), (33, 20, 13)]
ENGINE = (11, 1.5, "gaussian")
NULL = "NULL"                                              # the _win entries called with a NULL window
WANTS = ((True, True), (True, False), (False, True))
INF16 = {HM.F16: 0x7C00, HM.BF16: 0x7F80}


@pytest.fixture(scope="module")
def device(gpu_ctx):
    d = Device(gpu_ctx)
    yield d
    d.close()


def mk(window):
    """The ssim_amd.Window of a model window (size, sigma, kind)."""
    size, sigma, kind = window
    return ssim_amd.make_window(size, sigma if kind == "gaussian" else 1.5, kind)


def voxels(shape):
    return float(shape[2]) * float(shape[1]) * float(shape[0])


def constant_k(g_out, shape):
    """float(double(gOut) / (double(W) double(H) double(D))): the float the scalar form multiplies every voxel's derivatives by."""
    return np.float32(float(np.float32(g_out)) / voxels(shape))


def enqueue(ctx, enc, what, window, ps, n, r, *rest):
    """One enqueue of the family (enc None: float32; else 16-bit) `what` ("", "_grad", "_map_grad"): window None -- the entry without
    _win --, NULL -- the _win entry with a NULL window, through ctypes --, or a model window -- the _win entry through the binding."""
    name = "enqueue_ssim3%s%s" % ("f" if enc is None else "h", what)
    head = (ps, n, r) if enc is None else (ps, n, r, enc)
    if window is None:
        return call(getattr(ctx, name), *(head + rest))
    if window != NULL:
        return call(lambda: getattr(ctx, name)(*(head + rest), window=mk(window)))
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    fn = getattr(ctx.lib, "rmgr_ssim_hip_enqueue_ssim3%s_win%s" % ("f" if enc is None else "h", what))
    head = (ctx.handle, n, ps, r) if enc is None else (ctx.handle, n, ps, ssim_amd.sample_type_code(enc), r)
    rc = fn(*(head + (None,) + rest))
    if rc not in (0, 22):
        _device_error.append(rc)
    assert rc == 0, rc


def run(device, enc, pairs, r, window, g_out=None, gmaps=None, want=(True, True), maps=True, lin="dense", lout="dense", lmap=None, lg="dense"):
    """Forward (sums, maps) and backward of `pairs` under `window` in ONE enqueue each, device-resident.  enc None: the float32 entries
    on float32 volumes; else the ssim3h entries on uint16 bit patterns.  g_out: one dLoss/dS per pair (the _grad entry); gmaps: one
    float32 volume per pair, or one float per pair under the strides (0, 0, 0), under the layout lg (the _map_grad entry).  maps: True
    (every pair gets a map, under the layout lmap or lout), False, or {volume: layout}.  Returns (sums as float64, [map], [(dA or
    None, dB or None)])."""
    ctx, n = device.ctx, len(pairs)
    half = enc is not None
    dt = np.uint16 if half else np.float32
    PS, GR = (ssim_amd.Params3H, ssim_amd.Grad3H) if half else (ssim_amd.Params3F, ssim_amd.Grad3F)
    make = ssim_amd.make_params3h if half else ssim_amd.make_params3f
    d, h, w = pairs[0][0].shape
    arenas = []
    try:
        ins = Arena(dt)
        for a, b in pairs:
            ins.add(a.shape, lin, a)
            ins.add(b.shape, lin, b)
        arenas.append(ins.upload(ctx))
        mar = Arena(np.float32)
        map_at = dict(maps) if isinstance(maps, dict) else dict((i, lmap or lout) for i in range(n)) if maps else {}
        map_idx = dict((i, mar.add((d, h, w), map_at[i])) for i in sorted(map_at))
        arenas.append(mar.upload(ctx))
        sums = Arena(np.float64)
        sums.add((1, 1, n))
        arenas.append(sums.upload(ctx))
        ps = (PS * n)()
        for i in range(n):
            (pa, sa), (pb, sb) = ins.at(2 * i), ins.at(2 * i + 1)
            mp, ms = mar.at(map_idx[i]) if i in map_idx else (None, None)
            ps[i] = make(w, h, d, pa, sa, pb, sb, mp, ms)
        enqueue(ctx, enc, "", window, ps, n, r, sums.at(0)[0])
        backward = g_out is not None or gmaps is not None
        gar = Arena(dt)
        if backward:
            arrs, idx = [None, None], [[], []]
            for k in range(2):
                if want[k]:
                    for i in range(n):
                        idx[k].append(gar.add((d, h, w), lout))
            arenas.append(gar.upload(ctx))
            for k in range(2):
                if want[k]:
                    arrs[k] = (GR * n)()
                    for i in range(n):
                        p, s = gar.at(idx[k][i])
                        arrs[k][i] = GR(p, *s)
            up = Arena(np.float32)
            if g_out is not None:
                up.add((1, 1, n), "dense", np.asarray(g_out, np.float32).reshape(1, 1, n))
                arenas.append(up.upload(ctx))
                enqueue(ctx, enc, "_grad", window, ps, n, r, up.at(0)[0], arrs[0], arrs[1])
            else:
                gm = (ssim_amd.GradOut3F * n)()
                for i, k in enumerate(gmaps):
                    k = np.asarray(k, np.float32)
                    up.add((1, 1, 1) if k.ndim == 0 else k.shape, "dense" if k.ndim == 0 else lg, k)
                arenas.append(up.upload(ctx))
                for i, k in enumerate(gmaps):
                    p, s = up.at(i)
                    gm[i] = ssim_amd.GradOut3F(p, *((0, 0, 0) if np.ndim(k) == 0 else s))
                enqueue(ctx, enc, "_map_grad", window, ps, n, r, gm, arrs[0], arrs[1])
        call(ctx.synchronize)
        device.sample()
        s = sums.results()[0].reshape(n)
        ms = mar.results(written=True)                     # in ascending order of the volumes that have a map
        grads = []
        if backward:
            got = gar.results()
            grads = [(got[idx[0][i]] if want[0] else None, got[idx[1][i]] if want[1] else None) for i in range(n)]
            up.results()
        ins.results()                                      # the inputs and everything around them are unchanged
        return s, ms, grads
    finally:
        for a in arenas:
            a.free()


def check_against_float32(device, enc, pairs, r, window, what, **kw):
    """One call of the 16-bit entries against the same call of the float32 entries on the widened volumes under the same window: sums
    and maps bit for bit, gradients against the float32 gradients rounded once.  Returns (the 16-bit results, the float32 results)."""
    got = run(device, enc, pairs, r, window, **kw)
    ref = run(device, None, widened(pairs, enc), r, window, **kw)
    assert same64(got[0], ref[0]), (what, got[0], ref[0])
    assert len(got[1]) == len(ref[1])
    for m, wm in zip(got[1], ref[1]):
        assert HM.same_f32(m, wm), what
    assert len(got[2]) == len(ref[2])
    for (ga, gb), (fa, fb) in zip(got[2], ref[2]):
        for g, f in ((ga, fa), (gb, fb)):
            assert (g is None) == (f is None), what
            if g is not None:
                assert g.dtype == np.uint16 and HM.same(g, HM.round_to(f, enc), enc), what
    return got, ref


def same_grads(x, y):
    return all((p is None and q is None) or (p is not None and q is not None and np.array_equal(p, q)) for p, q in zip(x, y))


def normal_scale(device, enc, pair, r, window):
    """A dLoss/dS that puts the float16 gradients of this pair in the normal range: the largest float32 gradient magnitude becomes 1."""
    _, _, gr = run(device, None, widened([pair], enc), r, window, g_out=[1.0], maps=False)
    top = max(float(np.nanmax(np.abs(g))) for g in gr[0])
    return 1.0 / top if top > 0 else 1.0


# ---- value, map and sums; the blocking entries ---------------------------------------------------------------------------------------

@ENC
@WIN
def test_forward_has_the_bits_of_the_float32_windowed_path(device, window, enc):
    """fp64 sums and the map on every shape, the map also in a step-2 and a negative-sliceStride layout over a sentinel prefill; the
    blocking device and host entries (on the module's context, on a default context, in a batch) give the enqueue form's value and
    map; the windows differ from one another."""
    for shape in SHAPES:
        pair = IN.random_pair(shape, sum(shape), enc)
        for lmap in ("dense", "step 2", "negative sliceStride") if shape == (33, 20, 13) else ("dense",):
            (s, ms, _), _ = check_against_float32(device, enc, [pair], 1.0, window, ("forward", shape, lmap), lmap=lmap)
        want = np.float32(s[0] / voxels(pair[0].shape))
        (ha, st), (hb, _) = HM.host_array(pair[0], enc), HM.host_array(pair[1], enc)
        for ctx in (device.ctx, None):
            v, m = call(lambda: ssim_amd.compute_ssim3h(ha, hb, 1.0, st, True, ctx, window=mk(window)))
            assert np.float32(v).tobytes() == want.tobytes() and HM.same_f32(m, ms[0]), (shape, ctx)
        vs = call(lambda: ssim_amd.compute_ssim3h_batch([(ha, hb), (hb, ha)], 1.0, st, device.ctx, window=mk(window)))
        assert vs[:1].tobytes() == want.tobytes()
        d, h, w = pair[0].shape
        ins = Arena(np.uint16)
        ins.add(pair[0].shape, "dense", pair[0])
        ins.add(pair[1].shape, "dense", pair[1])
        ins.upload(device.ctx)
        try:
            ps = (ssim_amd.Params3H * 1)()
            ps[0] = ssim_amd.make_params3h(w, h, d, ins.at(0)[0], ins.at(0)[1], ins.at(1)[0], ins.at(1)[1])
            assert call(lambda: device.ctx.ssim3h_device(ps, 1, 1.0, enc, window=mk(window))).tobytes() == want.tobytes()
        finally:
            ins.free()
    assert not same64(run(device, enc, [pair], 1.0, None)[0], s)               # not the fixed window's result by accident


@ENC
@RADIUS
def test_host_entry_writes_the_map_through_arbitrary_strides(device, window, enc):
    """The C host entry with a float32 map at a step of 2, a stride of its own and a negative sliceStride: staged 2 bytes per sample,
    the map copied back at its strides, nothing beside it written."""
    a, b = IN.random_pair((21, 18, 7), 3, enc)
    (s, ms, _), _ = check_against_float32(device, enc, [(a, b)], 1.0, window, "dense")
    big = np.full((7, 18, 42), -777.0, np.float32)
    ps = (ssim_amd.Params3H * 1)()
    ps[0] = ssim_amd.make_params3h(21, 18, 7, a.ctypes.data, (1, 21, 21 * 18), b.ctypes.data, (1, 21, 21 * 18),
                                   big[::-1, :, 1::2].ctypes.data, (2, 42, -42 * 18))
    out = (ctypes.c_float * 1)()
    win = mk(window)
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    rc = device.ctx.lib.rmgr_ssim_hip_compute_ssim3h_win_host(device.ctx.handle, 1, ps, ssim_amd.sample_type_code(enc), 1.0, ctypes.byref(win), out)
    if rc not in (0, 22):
        _device_error.append(rc)
    assert rc == 0, rc
    assert np.float32(out[0]).tobytes() == np.float32(s[0] / voxels(a.shape)).tobytes()
    assert HM.same_f32(big[::-1, :, 1::2], ms[0]) and np.all(big[:, :, 0::2] == -777.0)


# ---- gradient and map gradient -------------------------------------------------------------------------------------------------------

@ENC
@WIN
def test_gradients_are_the_float32_gradients_rounded_once(device, window, enc):
    """dA alone, dB alone and both, with gOut scaled so that float16 gradients are normal numbers; each gradient has the same bits alone
    and together with the other; the map gradient under the constant gMap float(gOut / (W H D)) -- as a volume and as one float under
    strides (0, 0, 0) -- has the bits of the _win_grad entry under the same window."""
    for shape in SHAPES:
        pair = IN.random_pair(shape, 100 + sum(shape), enc)
        g = -0.75 * normal_scale(device, enc, pair, 1.0, window)
        (_, _, both), (_, _, f32) = check_against_float32(device, enc, [pair], 1.0, window, ("both", shape), g_out=[g], maps=False)
        (_, _, only_a), _ = check_against_float32(device, enc, [pair], 1.0, window, ("dA", shape), g_out=[g], want=(True, False), maps=False)
        (_, _, only_b), _ = check_against_float32(device, enc, [pair], 1.0, window, ("dB", shape), g_out=[g], want=(False, True), maps=False)
        assert np.array_equal(both[0][0], only_a[0][0]) and np.array_equal(both[0][1], only_b[0][1]) and only_a[0][1] is None and only_b[0][0] is None
        top = max(float(np.abs(f).max()) for f in f32[0])
        assert 0.7 < top < 0.8 or shape == (1, 1, 1), top                      # the scale did what it is for
        k = constant_k(g, pair[0].shape)
        for gm in (np.full(pair[0].shape, k, np.float32), k):
            for want in WANTS:
                _, _, ident = run(device, enc, [pair], 1.0, window, gmaps=[gm], want=want, maps=False)
                for side in range(2):
                    assert (ident[0][side] is None) == (not want[side])
                    if want[side]:
                        assert np.array_equal(ident[0][side], both[0][side]), (shape, want, side, np.ndim(gm))


@ENC
@WIN
def test_map_gradient_for_a_per_voxel_upstream_gradient(device, window, enc):
    """A random signed gMap under a mask, a one-hot gMap and one float under strides 0, for one gradient and for both: the float32 map
    gradient rounded once."""
    for shape in ((3, 5, 2), (33, 20, 13)):
        pair = IN.random_pair(shape, 11 + sum(shape), enc)
        rng = np.random.default_rng(12)
        gm = (rng.standard_normal(pair[0].shape) * (rng.random(pair[0].shape) < 0.6)).astype(np.float32)
        hot = np.zeros(pair[0].shape, np.float32)
        hot[tuple(s // 2 for s in hot.shape)] = 1000.0
        for k in (gm, hot, np.float32(0.03)):
            for want in WANTS:
                (_, _, gr), _ = check_against_float32(device, enc, [pair], 1.0, window, ("map grad", shape, want), gmaps=[k], want=want, maps=False)
        (_, _, gr), _ = check_against_float32(device, enc, [pair], 1.0, window, "one-hot", gmaps=[hot], maps=False)
        assert all(np.any(HM.widen(g, enc) != 0) for g in gr[0])


# ---- the identities with the fixed-window entries ------------------------------------------------------------------------------------

@ENC
@pytest.mark.parametrize("shape", [(17, 17, 9), (33, 20, 13)], ids=lambda s: "%dx%dx%d" % s)
def test_null_and_the_engine_window_give_the_bits_of_the_entries_without_win(device, enc, shape):
    pair = IN.random_pair(shape, 300 + sum(shape), enc)
    g = 0.5 * normal_scale(device, enc, pair, 1.0, None)
    gm = (np.random.default_rng(301).standard_normal(pair[0].shape) * 100).astype(np.float32)
    fixed = run(device, enc, [pair], 1.0, None, g_out=[g])
    fixed_map = run(device, enc, [pair], 1.0, None, gmaps=[gm], maps=False)[2]
    assert all(np.any(HM.widen(x, enc) != 0) for x in fixed[2][0] + fixed_map[0])
    for window in (ENGINE, NULL):
        got = run(device, enc, [pair], 1.0, window, g_out=[g])
        assert same64(got[0], fixed[0]) and HM.same_f32(got[1][0], fixed[1][0]) and same_grads(got[2][0], fixed[2][0]), window
        assert same_grads(run(device, enc, [pair], 1.0, window, gmaps=[gm], maps=False)[2][0], fixed_map[0]), window
    # the blocking _win entries with a NULL window
    d, h, w = pair[0].shape
    ins = Arena(np.uint16)
    ins.add(pair[0].shape, "dense", pair[0])
    ins.add(pair[1].shape, "dense", pair[1])
    ins.upload(device.ctx)
    try:
        ps = (ssim_amd.Params3H * 1)()
        ps[0] = ssim_amd.make_params3h(w, h, d, ins.at(0)[0], ins.at(0)[1], ins.at(1)[0], ins.at(1)[1])
        out = (ctypes.c_float * 1)()
        assert not _device_error, "an earlier call left a device error: %r" % _device_error
        rc = device.ctx.lib.rmgr_ssim_hip_compute_ssim3h_win_device(device.ctx.handle, 1, ps, ssim_amd.sample_type_code(enc), 1.0, None, out)
        if rc not in (0, 22):
            _device_error.append(rc)
        assert rc == 0 and np.float32(out[0]).tobytes() == np.float32(fixed[0][0] / voxels(pair[0].shape)).tobytes()
    finally:
        ins.free()


# ---- views ---------------------------------------------------------------------------------------------------------------------------

@ENC
@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "dense"])
def test_views_give_the_bits_of_the_dense_volume(device, enc, layout):
    """Negative, permuted, step 2, an odd 2-byte offset and stored (W, D, H), under every window: inputs, map, gradients and gMap under
    the layout against the dense call (which is held to the float32 path); every sentinel untouched (Arena.results)."""
    pair = IN.random_pair((21, 19, 14), 77, enc)
    gm = (np.random.default_rng(78).standard_normal(pair[0].shape) * 100).astype(np.float32)
    for window in WINDOWS:
        g = 0.5 * normal_scale(device, enc, pair, 1.0, window)
        dense, _ = check_against_float32(device, enc, [pair], 1.0, window, "dense", g_out=[g])
        dense_map, _ = check_against_float32(device, enc, [pair], 1.0, window, "dense gMap", gmaps=[gm], maps=False)
        for lin, lout in ((layout, "dense"), ("dense", layout), (layout, layout)):
            s, ms, gr = run(device, enc, [pair], 1.0, window, g_out=[g], lin=lin, lout=lout)
            assert same64(s, dense[0]) and HM.same_f32(ms[0], dense[1][0]) and same_grads(gr[0], dense[2][0]), (window, lin, lout)
        for lin, lg, lout in (("dense", layout, "dense"), (layout, layout, layout)):
            got = run(device, enc, [pair], 1.0, window, gmaps=[gm], maps=False, lin=lin, lg=lg, lout=lout)[2][0]
            assert same_grads(got, dense_map[2][0]), (window, lin, lg, lout)


# ---- content -------------------------------------------------------------------------------------------------------------------------

def _box(shape, where, radius):
    m = np.zeros(shape, bool)
    m[tuple(slice(max(p - radius, 0), p + radius + 1) for p in where)] = True
    return m


@ENC
@WIN
def test_the_reach_of_a_nan_is_the_windows(device, window, enc):
    """25 x 23 x 21, one NaN at the centre voxel (the centre then is 0) and at a corner.  A NaN sample: exactly the (2R + 1)^3 map voxels
    and the (4R + 1)^3 gradient voxels around it, clipped; a NaN in gMap: (2R + 1)^3 gradient voxels -- not 11^3 / 21^3.  Everything
    else is finite, and every finite bit is the float32 path's."""
    R = K2.radius(window)
    a, b = IN.random_pair((25, 23, 21), 5, enc)
    for where in ((10, 11, 12), (20, 0, 24)):
        an = a.copy()
        an[where] = NAN16[enc]
        (_, ms, gr), _ = check_against_float32(device, enc, [(an, b)], 1.0, window, "NaN sample", g_out=[1000.0])
        assert np.array_equal(np.isnan(ms[0]), _box(a.shape, where, R)) and np.all(np.isfinite(ms[0][~_box(a.shape, where, R)]))
        for g in gr[0]:
            assert np.array_equal(HM.is_nan(g, enc), _box(a.shape, where, 2 * R))
            assert np.all(np.isfinite(HM.widen(g, enc)[~_box(a.shape, where, 2 * R)]))
        gm = np.full(a.shape, 0.01, np.float32)
        gm[where] = np.nan
        (_, _, gr), _ = check_against_float32(device, enc, [(a, b)], 1.0, window, "NaN in gMap", gmaps=[gm], maps=False)
        for g in gr[0]:
            assert np.array_equal(HM.is_nan(g, enc), _box(a.shape, where, R))
            assert np.all(np.isfinite(HM.widen(g, enc)[~_box(a.shape, where, R)]))


@ENC
@WIN
def test_special_samples_at_the_centre_voxel(device, window, enc):
    """An Inf, a float16 subnormal and a sample above the data range at the centre voxel (17 x 17 x 9: voxel (4, 8, 8)), each in A, in
    B and in both: the float32 path's decision about the centre and its bits, NaN positions included.  A whole volume of subnormals of
    the encoding is not flushed."""
    a, b = IN.random_pair((17, 17, 9), 10, enc)
    sub = np.uint16(0x0155)                                 # a subnormal of float16; in bfloat16 a subnormal of float32 as well
    above = HM.round_to(np.float32([3.5]), enc)[0]
    for what, va, vb in (("Inf", INF16[enc], None), ("-Inf", None, INF16[enc] | 0x8000), ("subnormal", sub, sub), ("above the range", above, None),
                         ("above the range, both", above, HM.round_to(np.float32([-2.25]), enc)[0])):
        sa, sb = a.copy(), b.copy()
        if va is not None:
            sa[4, 8, 8] = va
        if vb is not None:
            sb[4, 8, 8] = vb
        (s, ms, gr), _ = check_against_float32(device, enc, [(sa, sb)], 1.0, window, what, g_out=[1000.0])
        if "Inf" in what:
            assert np.isnan(ms[0][4, 8, 8]) and not np.all(np.isnan(ms[0]))
        else:
            assert np.all(np.isfinite(ms[0])) and np.isfinite(s[0])
    rng = np.random.default_rng(9)
    top = 1023 if enc == HM.F16 else 127
    sa = rng.integers(1, top + 1, a.shape).astype(np.uint16)
    sb = np.clip(sa.astype(np.int32) + rng.integers(-40, 41, a.shape), 1, top).astype(np.uint16)
    assert np.all(HM.is_subnormal(sa, enc)) and np.all(HM.is_subnormal(sb, enc))
    r = float(HM.widen(np.uint16([1023]), HM.F16)[0]) if enc == HM.F16 else 1.0
    (s, _, _), _ = check_against_float32(device, enc, [(sa, sb)], r, window, "subnormals", g_out=[1.0])
    if enc == HM.F16:
        assert 0.0 < s[0] / voxels(a.shape) < 0.999                            # the samples were not flushed to zero: the pair differs


@ENC
@WIN
def test_subnormal_results_are_kept_and_overflow_gives_inf(device, window, enc):
    """Unscaled, the gradient of a mean SSIM is of order 1 / (W H D): among float16 subnormals, which are kept, not flushed.  Scaled far
    up -- the scale arrives in the float32 upstream gradient, before the single rounding -- some voxels overflow to Inf.  Both through
    the _win_grad and the _win_map_grad entry (bfloat16 has float32's exponent range: its overflow is reached through gMap)."""
    pair = IN.random_pair((33, 20, 13), 7, enc)
    (_, _, gr), (_, _, f32) = check_against_float32(device, enc, [pair], 1.0, window, "unscaled", g_out=[1.0], maps=False)
    if enc == HM.F16:
        for g in gr[0]:
            assert HM.is_subnormal(g, enc).sum() > 0                               # 1 / (W H D) = 1.2e-4: some voxels lie below 6.1e-5
    else:
        assert not np.any(HM.is_subnormal(gr[0][0], enc))
    vox = voxels(pair[0].shape)
    top = max(float(np.abs(f).max()) for f in f32[0]) * vox                    # the largest |gradient| per unit of k
    k = np.float32(min(4.0 * MAX16[enc] / top, 1.0e38))                       # a finite float32: bfloat16's range is float32's
    (_, _, gr), _ = check_against_float32(device, enc, [pair], 1.0, window, "overflow through gMap", gmaps=[k], maps=False)
    for g in gr[0]:
        inf = (g & 0x7FFF) == INF16[enc]
        print("%s %s: %d of %d voxels overflow to Inf at k = %g" % (K2.name_of(window), enc, int(inf.sum()), g.size, float(k)))
        assert inf.sum() < g.size and (inf.sum() > 0 or float(k) == 1.0e38), int(inf.sum())
    if enc == HM.F16:
        (_, _, gr2), _ = check_against_float32(device, enc, [pair], 1.0, window, "overflow through gOut", g_out=[float(k) * vox], maps=False)
        assert any(np.any((g & 0x7FFF) == 0x7C00) for g in gr2[0])


# ---- scheduling ----------------------------------------------------------------------------------------------------------------------

@ENC
@RADIUS
def test_deep_chunks_have_the_bits_of_the_lone_launch(device, window, enc):
    """17 x 17 x 131 alone (chunks of 8 slices) and inside a launch of enough volumes that plan3k of this radius, at the device's CU
    count, cuts z into chunks of at least 16 slices: the planner changes neither sums nor maps nor gradients nor map gradients.  The
    first, a middle and the last volume of the deep launch get a map, each in a layout of its own."""
    w, h, d = shape = (17, 17, 131)
    R = K2.radius(window)
    assert PK.plan3k(R, w, h, d, 1, device.cus).chunk_slices == 8
    n = next((n for n in range(2, 513) if PK.plan3k(R, w, h, d, n, device.cus).chunk_slices >= 16), None)
    assert n is not None, "no launch of up to 512 volumes of 17 x 17 x 131 reaches chunks of 16 slices on %d CUs at radius %d" % (device.cus, R)
    geo = PK.plan3k(R, w, h, d, n, device.cus)
    print("radius %d on %d CUs: %d volumes run at %r" % (R, device.cus, n, geo))
    assert geo.chunk_slices >= 16
    pairs = [IN.random_pair(shape, 50 + i, enc) for i in range(3)]
    gs = [0.75e4, -2.0e4, 0.5e4, 1.0e4]
    rng = np.random.default_rng(51)
    gms = [(rng.standard_normal(pairs[0][0].shape) * 10).astype(np.float32) for _ in range(2)]
    pick = [(i * 2 + i // 3) % 3 for i in range(n)]
    gpick = [(i * 3 + i // 4) % 4 for i in range(n)]
    mpick = [(i + i // 2) % 2 for i in range(n)]
    lone, lone_m, lone_fwd = {}, {}, []
    for k, pair in enumerate(pairs):
        (fs, fms, _), _ = check_against_float32(device, enc, [pair], 1.0, window, ("lone forward", k))
        lone_fwd.append((fs, fms[0]))
    for i in range(n):
        if (pick[i], gpick[i]) not in lone:
            lone[(pick[i], gpick[i])], _ = check_against_float32(device, enc, [pairs[pick[i]]], 1.0, window, "lone", g_out=[gs[gpick[i]]], maps=False)
        if (pick[i], mpick[i]) not in lone_m:
            lone_m[(pick[i], mpick[i])], _ = check_against_float32(device, enc, [pairs[pick[i]]], 1.0, window, "lone map", gmaps=[gms[mpick[i]]], maps=False)
    map_at = dict(zip(sorted(set((0, n // 2, n - 1))), ("dense", "step 2", "negative sliceStride")))
    assert len(map_at) == 3
    s, ms, gr = run(device, enc, [pairs[k] for k in pick], 1.0, window, g_out=[gs[k] for k in gpick], maps=map_at)
    assert len(ms) == 3
    for i, m in zip(sorted(map_at), ms):
        assert HM.same_f32(m, lone_fwd[pick[i]][1]), "the map of volume %d (pair %d, %s) of the deep launch" % (i, pick[i], map_at[i])
    _, _, gm = run(device, enc, [pairs[k] for k in pick], 1.0, window, gmaps=[gms[k] for k in mpick], maps=False)
    for i in range(n):
        want, want_m = lone[(pick[i], gpick[i])], lone_m[(pick[i], mpick[i])]
        assert same64(s[i:i + 1], want[0]) and same64(s[i:i + 1], lone_fwd[pick[i]][0]), i
        assert same_grads(gr[i], want[2][0]) and same_grads(gm[i], want_m[2][0]), i


@ENC
@WIN
def test_alone_or_anywhere_in_a_batch_and_on_a_second_call(device, window, enc):
    """A batch drawn from several pairs and gOut values, in two orders, twice: each volume has the bits of its lone call."""
    size = (33, 20, 13)
    pairs = [IN.random_pair(size, 40 + i, enc) for i in range(3)]
    g = [-0.75e4, 1.5e4, 0.25e4]
    rng = np.random.default_rng(41)
    gms = [rng.standard_normal(pairs[0][0].shape).astype(np.float32) for _ in range(3)]
    alone = [run(device, enc, [pairs[i]], 1.0, window, g_out=[g[i]]) for i in range(3)]
    alone_m = [run(device, enc, [pairs[i]], 1.0, window, gmaps=[gms[i]], maps=False) for i in range(3)]
    check_against_float32(device, enc, pairs, 1.0, window, "the batch", g_out=g)
    for order in ((0, 1, 2), (2, 0, 1)):
        for again in range(2):
            s, ms, gr = run(device, enc, [pairs[i] for i in order], 1.0, window, g_out=[g[i] for i in order])
            _, _, gm = run(device, enc, [pairs[i] for i in order], 1.0, window, gmaps=[gms[i] for i in order], maps=False)
            for pos, i in enumerate(order):
                assert same64(s[pos:pos + 1], alone[i][0]) and HM.same_f32(ms[pos], alone[i][1][0]), (order, pos, again)
                assert same_grads(gr[pos], alone[i][2][0]) and same_grads(gm[pos], alone_m[i][2][0]), (order, pos, again)


@ENC
@RADIUS
def test_enqueues_beyond_the_ring_keep_their_order(device, window, enc):
    """17 different pairs of 33 x 17 x 9: one forward and one gradient enqueue each, back to back -- 34 launches from the ring of 8
    descriptor slots -- and one synchronise: the lone results."""
    ctx, (w, h, d), n = device.ctx, (33, 17, 9), 17
    vox = w * h * d
    win = mk(window)
    pairs = [IN.random_pair((w, h, d), 60 + i, enc) for i in range(n)]
    g_out = np.float32([(-0.75e4, 0.5e4, 1.0e4)[i % 3] for i in range(n)])
    lone = [run(device, enc, [pairs[i]], 1.0, window, g_out=[g_out[i]], maps=False) for i in range(n)]
    assert len(set(x[0].tobytes() for x in lone)) == n
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    bufs = [(ctx.upload(a), ctx.upload(b)) for a, b in pairs]
    per = vox + GAP
    fresh = np.full(2 * n * per + GAP, SENT[np.dtype(np.uint16)], np.uint16)
    out, sums, go = ctx.upload(fresh), ctx.upload(np.full(n + 2, -777.0)), ctx.upload(g_out)
    try:
        keep = []
        for i in range(n):
            ps, ga, gb = (ssim_amd.Params3H * 1)(), (ssim_amd.Grad3H * 1)(), (ssim_amd.Grad3H * 1)()
            ps[0] = ssim_amd.make_params3h(w, h, d, bufs[i][0].ptr, (1, w, w * h), bufs[i][1].ptr, (1, w, w * h))
            ga[0] = ssim_amd.Grad3H(out.ptr + 2 * (GAP + 2 * i * per), 1, w, w * h)
            gb[0] = ssim_amd.Grad3H(out.ptr + 2 * (GAP + (2 * i + 1) * per), 1, w, w * h)
            keep.append((ps, ga, gb))
            call(lambda: ctx.enqueue_ssim3h(ps, 1, 1.0, enc, sums.ptr + 8 * (1 + i), window=win))
            call(lambda: ctx.enqueue_ssim3h_grad(ps, 1, 1.0, enc, go.ptr + 4 * i, ga, gb, window=win))
        call(ctx.synchronize)
        device.sample()
        s = sums.download(np.float64, (n + 2,))
        assert s[0] == -777.0 and s[-1] == -777.0
        host = out.download(np.uint16, fresh.shape)
        body = host[GAP:].reshape(2 * n, per)
        assert np.all(host[:GAP] == fresh[0]) and np.all(body[:, vox:] == fresh[0]), "a gap between the gradient volumes changed"
        for i in range(n):
            assert same64(s[1 + i:2 + i], lone[i][0]), i
            for side in range(2):
                assert np.array_equal(body[2 * i + side, :vox].reshape(d, h, w), lone[i][2][0][side]), (i, side)
    finally:
        for x in [out, sums, go] + [b for ab in bufs for b in ab]:
            x.free()


@ENC
def test_windowed_16_bit_calls_share_one_context_with_the_other_volume_calls(device, enc):
    """On one context, 30 enqueues alternate without a host wait, with trim() after the fifteenth: forward, gradient and map gradient of
    16-bit volumes under five windows (every radius), interleaved with float32 windowed calls and with fixed-window calls of both
    families -- more than the 8 descriptor slots, every backward rewriting the shared coefficient scratch.  Every output has the bytes
    of the same call issued alone, with a host wait, on another context."""
    ctx = device.ctx
    shapes = [(33, 20, 13), (20, 18, 40)]
    data = []
    for i, size in enumerate(shapes):
        a, b = IN.random_pair(size, 200 + i, enc)
        k = (np.random.default_rng(210 + i).standard_normal(a.shape) * 100).astype(np.float32)
        data.append(dict(h=(ctx.upload(a), ctx.upload(b)), f=(ctx.upload(HM.widen(a, enc)), ctx.upload(HM.widen(b, enc))), k=ctx.upload(k),
                         go=ctx.upload(np.float32([-0.75e4 + 1e4 * i])), shape=a.shape))
    kinds = []
    for j, win in enumerate(ONE_PER_RADIUS):
        kinds += [(0, "forward", "h", win), (1, "grad", "h", win), (0, "map_grad", "h", win),
                  (1, ("forward", "grad", "map_grad")[j % 3], "f", win), (j % 2, ("grad", "map_grad", "forward")[j % 3], "h", None),
                  (1 - j % 2, ("map_grad", "forward", "grad")[j % 3], "f", None)]
    assert len(kinds) == 30

    def issue(c, wait, trim_after=None):
        outs, keep = [], []
        for shape_i, what, fam, _ in kinds:                 # the outputs first: an upload waits for its context's stream
            vox = int(np.prod(data[shape_i]["shape"]))
            es = 4 if fam == "f" or what == "forward" else 2
            outs.append((ctx.upload(np.full(1, -777.0)), ctx.upload(np.full(vox, -777.0, np.float32))) if what == "forward"
                        else (ctx.upload(np.zeros(vox * es, np.uint8)), ctx.upload(np.zeros(vox * es, np.uint8))))
        call(ctx.synchronize)
        for pos, ((shape_i, what, fam, win), out) in enumerate(zip(kinds, outs)):
            item = data[shape_i]
            d, h, w = item["shape"]
            dense = (1, w, w * h)
            PS, GR, make = (ssim_amd.Params3F, ssim_amd.Grad3F, ssim_amd.make_params3f) if fam == "f" else (ssim_amd.Params3H, ssim_amd.Grad3H, ssim_amd.make_params3h)
            va, vb = item[fam]
            ps = (PS * 1)()
            kw = {} if win is None else {"window": mk(win)}
            head = (ps, 1, 1.0) if fam == "f" else (ps, 1, 1.0, enc)
            if what == "forward":
                ps[0] = make(w, h, d, va.ptr, dense, vb.ptr, dense, out[1].ptr, dense)
                call(lambda: getattr(c, "enqueue_ssim3" + fam)(*(head + (out[0].ptr,)), **kw))
            else:
                ps[0] = make(w, h, d, va.ptr, dense, vb.ptr, dense)
                pa, pb = (GR * 1)(), (GR * 1)()
                pa[0], pb[0] = GR(out[0].ptr, *dense), GR(out[1].ptr, *dense)
                keep.extend((pa, pb))
                if what == "grad":
                    call(lambda: getattr(c, "enqueue_ssim3%s_grad" % fam)(*(head + (item["go"].ptr, pa, pb)), **kw))
                else:
                    ms = (ssim_amd.GradOut3F * 1)()
                    ms[0] = ssim_amd.GradOut3F(item["k"].ptr, *dense)
                    keep.append(ms)
                    call(lambda: getattr(c, "enqueue_ssim3%s_map_grad" % fam)(*(head + (ms, pa, pb)), **kw))
            keep.append(ps)
            if wait:
                call(c.synchronize)
            if trim_after == pos:
                c.trim()
        call(c.synchronize)
        device.sample()
        got = []
        for (shape_i, what, fam, _), out in zip(kinds, outs):
            vox = int(np.prod(data[shape_i]["shape"]))
            es = 4 if fam == "f" or what == "forward" else 2
            got.append((out[0].download(np.float64, (1,)).tobytes(), out[1].download(np.float32, (vox,)).tobytes()) if what == "forward"
                       else (out[0].download(np.uint8, (vox * es,)).tobytes(), out[1].download(np.uint8, (vox * es,)).tobytes()))
            out[0].free()
            out[1].free()
        return got
    try:
        call(ctx.synchronize)                               # the uploads above, before another context's stream reads them
        with ssim_amd.Context(0) as other:
            alone = issue(other, True)
        mixed = issue(ctx, False, trim_after=14)
        for i, kind in enumerate(kinds):
            assert mixed[i] == alone[i], (i, kind)
            assert any(alone[i][1]) and alone[i][1] != np.full(len(alone[i][1]) // 4, -777.0, np.float32).tobytes(), (i, kind)
        assert alone[0][1] != alone[6][1] and alone[6][1] != alone[12][1]      # the windows differ: no call was compared with itself by accident
    finally:
        for item in data:
            for v in item["h"] + item["f"] + (item["k"], item["go"]):
                v.free()


# ---- PyTorch -------------------------------------------------------------------------------------------------------------------------
# torch brings its own HIP runtime; the checks run in ONE child process (tests/tools/ssim3hk_torch_checks.py) that imports torch before
# the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    tool = os.path.join(ROOT, "tests", "tools", "ssim3hk_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "ssim3hk_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["value_and_gradient_are_the_float32_windowed_path_rounded_once", "non_contiguous_expanded_and_y_only",
                                   "side_stream", "sum_of_the_map_and_a_scaled_loss", "default_keywords_are_the_call_without_keywords",
                                   "ssim3d_still_refuses_16_bit_tensors"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
