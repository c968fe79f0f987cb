"""GPU: SSIM of float16 / bfloat16 planes under a caller-chosen window, its gradient and the gradient of its map
(rmgr_ssim_hip_*_ssimh_win*; ssimhk_kernels.hip for 3, 5, 7 and 9 taps, ssimh_kernels.hip / ssimw_kernels.hip with the window's taps for
11) against the float32 _win entries, BIT FOR BIT.  Sizes are W x H; arrays are (H, W); 16-bit samples travel as uint16 bit patterns.

The contract (include/rmgr/ssim-hip.h): value, map and fp64 sums have the bits rmgr_ssim_hip_enqueue_ssimf_win gives on the widened
planes under the same window; a gradient pixel is the float32 value of _enqueue_ssimf_win_grad / _ssimf_win_map_grad rounded once, to
nearest-even, into the inputs' encoding.  So every comparison here runs the float32 _win entry in the same test on
halfmodel.widen(samples) and compares bits -- gradients against halfmodel.round_to(float32 gradient) -- and no tolerance is new; NaN is
compared as NaN.  No float64 model runs here: tests/test_gpu_ssimk.py holds the float32 windowed path to tests/ssimk_model.py, and bit
equality carries that over.

Windows: the seven of ssimk_model.WINDOWS -- every radius kernel, and the 11-tap route with foreign taps --, or one per radius where a
sweep is expensive.  Shapes: 1 x 1, 2 x 1, 1 x 2, 5 x 3, 4 x 4, 9 x 9 (borders inside the radius), 33 x 33 (a tile edge), 129 x 17 (a second
128-column strip column, a 64-column cell edge), 7 x 300 (several 32-row cells); 300 pairs of 9 x 603 for strips of many cells.

After a return code that is neither success nor EINVAL the module starts nothing more on the GPU (test_gpu_ssimk's _ok / _device_error,
shared with that module).  The module prints its wall time and its peak device memory when it ends.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import halfmodel as HM
import sample_forms_inputs as SF
import ssimhk_inputs as IN
import ssimk_model as K
import ssim_amd
from conftest import ROOT
from test_gpu_ssimk import _device_error, _ok, _sync, mk, same64
from test_gpu_ssimw import FILL16, FILL32, Plane

pytestmark = pytest.mark.gpu

ENC = pytest.mark.parametrize("enc", HM.ENCODINGS)
WINDOWS = K.WINDOWS
WIN = pytest.mark.parametrize("window", WINDOWS, ids=[K.name_of(w) for w in WINDOWS])
ONE_PER_RADIUS = IN.ONE_PER_RADIUS
RADIUS = pytest.mark.parametrize("window", ONE_PER_RADIUS, ids=[K.name_of(w) for w in ONE_PER_RADIUS])
SIZES = ((1, 1), (2, 1), (1, 2), (5, 3), (4, 4), (9, 9), (33, 33), (129, 17), (7, 300))
ENGINE = (11, 1.5, "gaussian")
NULL = "NULL"                                              # the _win entries called with a NULL window
NAN16 = {HM.F16: 0x7E00, HM.BF16: 0x7FC0}
INF16 = {HM.F16: 0x7C00, HM.BF16: 0x7F80}
MAX16 = {HM.F16: 65504.0, HM.BF16: 3.3895313892515355e38}


class Device(object):
    def __init__(self, ctx):
        self.ctx, self.t0 = ctx, time.time()
        self.free0 = self.min_free = ssim_amd.memory_info(ctx)[0]

    def sample(self):
        self.min_free = min(self.min_free, ssim_amd.memory_info(self.ctx)[0])

    def close(self):
        self.ctx.trim()
        print("\nwindowed 16-bit planes: module wall time %.1f s; peak device memory in use by the module %.1f MiB" % (
            time.time() - self.t0, (self.free0 - self.min_free) / 2.0 ** 20))


@pytest.fixture(scope="module")
def device(gpu_ctx):
    d = Device(gpu_ctx)
    yield d
    d.close()


def entry(ctx, enc, name, window):
    """The C entry `name` ("enqueue_ssim%s", "compute_ssim%s_device", "enqueue_ssim%s_grad", "enqueue_ssim%s_map_grad") of the family
    (enc None: float32; else 16-bit) as f(n, ps, r, *rest): window None -- the entry without _win --, NULL -- the _win entry with a NULL
    window --, or a model window -- the _win entry under it."""
    fam = "f" if enc is None else "h"
    plain = name % fam
    head = (ctx.handle,)

    def f(n, ps, r, *rest):
        assert not _device_error, "an earlier call left a device error: %r" % _device_error
        pre = head + (n, ps) + (() if enc is None else (ssim_amd.sample_type_code(enc),)) + (r,)
        if window is None:
            return _ok(getattr(ctx.lib, "rmgr_ssim_hip_" + plain)(*(pre + rest)))
        win = None if window == NULL else mk(window)
        wname = plain.replace("ssim" + fam, "ssim%s_win" % fam)
        return _ok(getattr(ctx.lib, "rmgr_ssim_hip_" + wname)(*(pre + (None if win is None else ctypes.byref(win),) + rest)))
    return f


def run(device, enc, pairs, r, window, g_out=None, gmaps=None, which=3, maps=True, step=1, flip=False, blocking=False):
    """Forward (sums, maps) and backward of `pairs` under `window` in ONE enqueue each, device-resident, every plane in the layout (step,
    flip) of test_gpu_ssimw.Plane.  enc None: the float32 entries on float32 planes; else the ssimh entries on uint16 bit patterns.
    g_out: one dLoss/dS per pair (the _grad entry); gmaps: one float32 plane per pair, or one float per pair behind step = stride = 0
    (the _map_grad entry).  blocking: the forward through _compute_*_device (float32 values instead of sums).  Returns (sums as float64
    or values as float32, [map], [(dA or None, dB or None)])."""
    ctx, n = device.ctx, len(pairs)
    half = enc is not None
    dt, fill = (np.uint16, FILL16) if half else (np.float32, FILL32)
    PS, GR = (ssim_amd.Params16, ssim_amd.GradH) if half else (ssim_amd.ParamsF, ssim_amd.GradF)
    make = ssim_amd.make_params16 if half else ssim_amd.make_params_f
    h, w = pairs[0][0].shape
    made, bufs = [], []

    def plane(arr, **kw):
        made.append(Plane(ctx, arr, step=step, flip=flip, **kw))
        return made[-1]
    try:
        ps, mplanes = (PS * n)(), []
        for i, (a, b) in enumerate(pairs):
            pa, pb = plane(np.asarray(a, dt)), plane(np.asarray(b, dt))
            if maps:
                m = plane(np.full((h, w), FILL32, np.float32), fill=FILL32)
                mplanes.append(m)
                ps[i] = make(w, h, pa.ptr, pa.dstep, pa.dstride, pb.ptr, pb.dstep, pb.dstride, m.ptr, m.dstep, m.dstride)
            else:
                ps[i] = make(w, h, pa.ptr, pa.dstep, pa.dstride, pb.ptr, pb.dstep, pb.dstride)
        if blocking:
            out = (ctypes.c_float * n)()
            entry(ctx, enc, "compute_ssim%s_device", window)(n, ps, r, out)
            values = np.array(out[:n], np.float32)
        else:
            sums = ctx.upload(np.full(n, -777.0))
            bufs.append(sums)
            entry(ctx, enc, "enqueue_ssim%s", window)(n, ps, r, sums.ptr)
        arrs, outs = [None, None], [[], []]
        if g_out is not None or gmaps is not None:
            for k in range(2):
                if which & (1 << k):
                    arrs[k] = (GR * n)()
                    for i in range(n):
                        g = plane(np.full((h, w), fill, dt), fill=fill)
                        outs[k].append(g)
                        arrs[k][i] = GR(g.ptr, g.dstep, g.dstride)
            if g_out is not None:
                go = ctx.upload(np.asarray(g_out, np.float32))
                bufs.append(go)
                entry(ctx, enc, "enqueue_ssim%s_grad", window)(n, ps, r, go.ptr, arrs[0], arrs[1])
            else:
                ms = (ssim_amd.GradOutF * n)()
                for i, k in enumerate(gmaps):
                    if np.ndim(k) == 0:
                        one = ctx.upload(np.float32([k]))
                        bufs.append(one)
                        ms[i] = ssim_amd.GradOutF(one.ptr, 0, 0)
                    else:
                        m = plane(np.asarray(k, np.float32))
                        ms[i] = ssim_amd.GradOutF(m.ptr, m.dstep, m.dstride)
                entry(ctx, enc, "enqueue_ssim%s_map_grad", window)(n, ps, r, ms, arrs[0], arrs[1])
        _sync(ctx)
        device.sample()
        if not blocking:
            values = sums.download(np.float64, (n,))
        got_maps = [m.read() for m in mplanes]
        grads = [tuple(outs[k][i].read() if arrs[k] is not None else None for k in range(2)) for i in range(n)] if arrs != [None, None] else []
        return values, got_maps, grads
    finally:
        for p in made + bufs:
            p.free()


def check_against_float32(device, enc, pairs, r, window, what, **kw):
    """One call of the 16-bit entries against the same call of the float32 entries on the widened planes under the same window: sums
    and maps bit for bit, gradients against the float32 gradients rounded once.  Returns (the 16-bit results, the float32 results)."""
    got = run(device, enc, pairs, r, window, **kw)
    ref = run(device, None, IN.widened(pairs, enc), r, window, **kw)
    assert got[0].dtype == ref[0].dtype and got[0].tobytes() == ref[0].tobytes(), (what, got[0], ref[0])
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


def pixels(shape):
    return float(shape[1]) * float(shape[0])


def constant_k(g_out, shape):
    """float(double(gOut) / (double(W) double(H))): the float the scalar form multiplies every pixel's derivatives by."""
    return np.float32(float(np.float32(g_out)) / pixels(shape))


# ---- value, map and sums; the blocking entries ---------------------------------------------------------------------------------------

@ENC
@WIN
def test_forward_has_the_bits_of_the_float32_windowed_path(device, window, enc):
    """fp64 sums and the map on every shape; the blocking device and host entries (on the module's context, on a default context, in a
    batch, through the binding's keyword) give the enqueue form's value and map; the result is not the fixed window's."""
    for w, h in SIZES:
        pair = IN.random_pair(w, h, 100 * w + h, enc)
        (s, ms, _), _ = check_against_float32(device, enc, [pair], 1.0, window, ("forward", w, h))
        want = np.float32(s[0] / pixels(pair[0].shape))
        (v, ms2, _), _ = check_against_float32(device, enc, [pair], 1.0, window, ("device", w, h), blocking=True)
        assert v[:1].tobytes() == want.tobytes() and HM.same_f32(ms2[0], ms[0]), (w, h)
        (ha, st), (hb, _) = HM.host_array(pair[0], enc), HM.host_array(pair[1], enc)
        for ctx in (device.ctx, None):
            hv, hm = ssim_amd.compute_ssimh(ha, hb, 1.0, st, True, ctx, window=mk(window))
            assert np.float32(hv).tobytes() == want.tobytes() and HM.same_f32(hm, ms[0]), (w, h, ctx)
        vs = ssim_amd.compute_ssimh_batch([(ha, hb), (hb, ha)], 1.0, st, device.ctx, window=mk(window))
        assert vs[:1].tobytes() == want.tobytes()
        da, db = device.ctx.upload(pair[0]), device.ctx.upload(pair[1])
        try:
            ps = (ssim_amd.Params16 * 1)(ssim_amd.make_params16(w, h, da.ptr, 1, w, db.ptr, 1, w))
            assert device.ctx.ssimh_device(ps, 1, 1.0, enc, window=mk(window)).tobytes() == want.tobytes()
        finally:
            da.free()
            db.free()
    pair = IN.random_pair(33, 33, 3333, enc)
    s, ms, _ = run(device, enc, [pair], 1.0, window)
    fixed = run(device, enc, [pair], 1.0, None)
    assert not same64(fixed[0], s) and not HM.same_f32(fixed[1][0], ms[0])     # not the fixed window's result: no silent fall-back


# ---- gradient and map gradient -------------------------------------------------------------------------------------------------------

@ENC
@WIN
def test_gradients_are_the_float32_gradients_rounded_once(device, window, enc):
    """dA alone, dB alone and both, with gOut = W H so that float16 gradients are normal numbers; each gradient has the same bits alone and
    together with the other; the map gradient under the constant gMap float(gOut / (W H)) -- as a plane and as one float behind strides
    (0, 0) -- has the bits of the _win_grad entry under the same window."""
    for w, h in SIZES:
        pair = IN.random_pair(w, h, 200 * w + h, enc)
        g = -0.75 * w * h
        (_, _, both), _ = check_against_float32(device, enc, [pair], 1.0, window, ("both", w, h), g_out=[g], maps=False)
        (_, _, only_a), _ = check_against_float32(device, enc, [pair], 1.0, window, ("dA", w, h), g_out=[g], which=1, maps=False)
        (_, _, only_b), _ = check_against_float32(device, enc, [pair], 1.0, window, ("dB", w, h), g_out=[g], which=2, maps=False)
        assert np.array_equal(both[0][0], only_a[0][0]) and np.array_equal(both[0][1], only_b[0][1]) and only_a[0][1] is None and only_b[0][0] is None
        if (w, h) != (1, 1):
            assert all(np.any((x & 0x7FFF) != 0) for x in both[0]), (w, h)
        k = constant_k(g, pair[0].shape)
        for gm in (np.full(pair[0].shape, k, np.float32), k):
            for which in (3, 1, 2):
                _, _, ident = run(device, enc, [pair], 1.0, window, gmaps=[gm], which=which, maps=False)
                for side in range(2):
                    assert (ident[0][side] is None) == (not which & (1 << side))
                    if which & (1 << side):
                        assert np.array_equal(ident[0][side], both[0][side]), (w, h, which, side, np.ndim(gm))


@ENC
@WIN
def test_map_gradient_for_a_per_pixel_upstream_gradient(device, window, enc):
    """A standard normal gMap, the same under a mask, a one-hot gMap and one float behind strides 0, for one gradient and for both: the
    float32 map gradient rounded once."""
    for w, h in ((5, 3), (33, 33), (129, 17)):
        pair = IN.random_pair(w, h, 300 * w + h, enc)
        rng = np.random.default_rng(12)
        normal = rng.standard_normal(pair[0].shape).astype(np.float32)
        masked = (normal * (rng.random(pair[0].shape) < 0.6)).astype(np.float32)
        hot = np.zeros(pair[0].shape, np.float32)
        hot[h // 2, w // 2] = 1000.0
        for k in (normal, masked, hot, np.float32(0.03)):
            for which in (3, 1, 2):
                (_, _, gr), _ = check_against_float32(device, enc, [pair], 1.0, window, ("map grad", w, h, which), gmaps=[k], which=which, maps=False)
        (_, _, gr), _ = check_against_float32(device, enc, [pair], 1.0, window, "one-hot", gmaps=[hot], maps=False)
        assert all(np.any(HM.widen(g, enc) != 0) for g in gr[0])


# ---- the identities with the fixed-window entries ------------------------------------------------------------------------------------

@ENC
@pytest.mark.parametrize("size", [(1, 1), (33, 33), (129, 17)], ids=lambda s: "%dx%d" % s)
def test_null_and_the_engine_window_give_the_bits_of_the_entries_without_win(device, enc, size):
    w, h = size
    pairs = [IN.random_pair(w, h, 7, enc), IN.random_pair(w, h, 8, enc)]
    g = [-0.75 * w * h, 0.5 * w * h]
    gms = [(np.random.default_rng(301 + i).standard_normal((h, w)) * 100).astype(np.float32) for i in range(2)]
    fixed = run(device, enc, pairs, 1.0, None, g_out=g)
    fixed_v = run(device, enc, pairs, 1.0, None, blocking=True)
    fixed_map = run(device, enc, pairs, 1.0, None, gmaps=gms, maps=False)[2]
    assert all(np.any(HM.widen(x, enc) != 0) for x in fixed[2][1] + fixed_map[1])
    for window in (ENGINE, NULL):
        got = run(device, enc, pairs, 1.0, window, g_out=g)
        assert same64(got[0], fixed[0]) and all(HM.same_f32(x, y) for x, y in zip(got[1], fixed[1])), window
        assert all(same_grads(x, y) for x, y in zip(got[2], fixed[2])), window
        gv = run(device, enc, pairs, 1.0, window, blocking=True)
        assert gv[0].tobytes() == fixed_v[0].tobytes() and all(HM.same_f32(x, y) for x, y in zip(gv[1], fixed_v[1])), window
        assert all(same_grads(x, y) for x, y in zip(run(device, enc, pairs, 1.0, window, gmaps=gms, maps=False)[2], fixed_map)), window
        # the host entry itself, with this window (NULL included), and the binding's keyword
        a, b = pairs[0]
        out, m = (ctypes.c_float * 1)(), np.empty((h, w), np.float32)
        ps = (ssim_amd.Params16 * 1)(ssim_amd.make_params16(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w, m.ctypes.data, 1, w))
        win = None if window == NULL else mk(window)
        _ok(device.ctx.lib.rmgr_ssim_hip_compute_ssimh_win_host(device.ctx.handle, 1, ps, ssim_amd.sample_type_code(enc), 1.0,
                                                                None if win is None else ctypes.byref(win), out))
        assert np.float32(out[0]).tobytes() == fixed_v[0][:1].tobytes() and HM.same_f32(m, fixed[1][0])
        (ha, st), (hb, _) = HM.host_array(a, enc), HM.host_array(b, enc)
        hv, hm = ssim_amd.compute_ssimh(ha, hb, 1.0, st, True, device.ctx, window=win)
        assert np.float32(hv).tobytes() == fixed_v[0][:1].tobytes() and HM.same_f32(hm, fixed[1][0])


# ---- views ---------------------------------------------------------------------------------------------------------------------------

@ENC
@WIN
def test_views_give_the_bits_of_the_dense_planes(device, window, enc):
    """Samples, map, upstream planes and gradient planes interleaved (step 3), stored back to front behind negative steps, and both
    (Plane.read asserts that the gaps of a strided output plane still hold their fill); then the C host entry with a float32 map at a
    step of 2 and a stride of its own: staged 2 bytes per sample, the map copied back at its strides, nothing beside it written."""
    w, h = 129, 17
    pair = IN.random_pair(w, h, 4, enc)
    gm = (np.random.default_rng(78).standard_normal((h, w)) * 100).astype(np.float32)
    g = 0.5 * w * h
    dense, _ = check_against_float32(device, enc, [pair], 1.0, window, "dense", g_out=[g])
    dense_map, _ = check_against_float32(device, enc, [pair], 1.0, window, "dense gMap", gmaps=[gm], maps=False)
    for step, flip in ((3, False), (1, True), (2, True)):
        s, ms, gr = run(device, enc, [pair], 1.0, window, g_out=[g], step=step, flip=flip)
        assert same64(s, dense[0]) and HM.same_f32(ms[0], dense[1][0]) and same_grads(gr[0], dense[2][0]), (step, flip)
        got = run(device, enc, [pair], 1.0, window, gmaps=[gm], maps=False, step=step, flip=flip)[2][0]
        assert same_grads(got, dense_map[2][0]), (step, flip)
    a, b = pair
    big = np.full((h, 2 * w + 6), -777.0, np.float32)
    ra = np.ascontiguousarray(a[::-1, ::-1])                # A stored back to front, read through negative steps
    ps = (ssim_amd.Params16 * 1)(ssim_amd.make_params16(w, h, ra.ctypes.data + 2 * (h * w - 1), -1, -w, b.ctypes.data, 1, w,
                                                        big[:, 1::2].ctypes.data, 2, 2 * w + 6))
    out, win = (ctypes.c_float * 1)(), mk(window)
    _ok(device.ctx.lib.rmgr_ssim_hip_compute_ssimh_win_host(device.ctx.handle, 1, ps, ssim_amd.sample_type_code(enc), 1.0, ctypes.byref(win), out))
    assert np.float32(out[0]).tobytes() == np.float32(dense[0][0] / pixels(a.shape)).tobytes()
    assert HM.same_f32(big[:, 1:2 * w + 1:2], dense[1][0]) and np.all(big[:, 0::2] == -777.0) and np.all(big[:, 2 * w + 1:] == -777.0)


# ---- the 64-bit forms ----------------------------------------------------------------------------------------------------------------

@ENC
@pytest.mark.parametrize("window", [(3, 0.0, "uniform"), (11, 2.0, "gaussian")], ids=K.name_of)
def test_64_bit_forms(device, window, enc):
    """Samples and gradient planes 2^22 two-byte elements apart, the map and the upstream plane 2^21 floats apart (fitsh_narrow() fails:
    the kernels' 64-bit lane offsets), read in either direction: the bits of the dense call, which is held to the float32 path.  Nothing
    but the output planes changes in either volume."""
    from test_gpu_sample_forms import Volume
    ctx, win = device.ctx, mk(window)
    w, h = 9, 12
    a, b = IN.random_pair(w, h, 64, enc)
    gmap = (np.random.default_rng(65).standard_normal((h, w)) * 10).astype(np.float32)
    g = -0.75 * w * h
    dense, _ = check_against_float32(device, enc, [(a, b)], 1.0, window, "dense", g_out=[g])
    dense_map, _ = check_against_float32(device, enc, [(a, b)], 1.0, window, "dense gMap", gmaps=[gmap], maps=False)
    lay16, lay32 = SF.Layout(np.uint16, SF.EDGE_H, w), SF.Layout(np.float32, SF.EDGE, w)
    lay16.add("a", a)
    lay16.add("b", b)
    lay32.add("g", gmap)
    lay16.close(out_rows=3 * 4 * h)
    lay32.close(out_rows=3 * h)
    vol16, vol32 = None, None
    go, sums = ctx.upload(np.float32([g])), ctx.upload(np.full(1, -777.0))
    try:
        vol16 = Volume(ctx, lay16, np.uint16(NAN16[enc]), np.uint16(FILL16))
        vol32 = Volume(ctx, lay32, np.float32(-3.0), FILL32)
        device.sample()
        done = []
        for fx, fy in ((False, False), (True, True), (True, False)):
            ia, ib, ig = vol16.src("a", fx, fy), vol16.src("b", fy, fx), vol32.src("g", fx, fx)
            assert abs(ia[1]) >= 1 << 22 and abs(ig[1]) >= 1 << 21
            om = vol32.dst(h, w, fx, fy)
            oa, ob, pa, pb = (vol16.dst(h, w, f1, f2) for f1, f2 in ((fy, fx), (fx, fx), (fy, fy), (not fx, fy)))
            assert abs(om.triple[1]) >= 1 << 21 and abs(oa.triple[1]) >= 1 << 21
            ps = (ssim_amd.Params16 * 1)(ssim_amd.make_params16(w, h, ia[0], ia[1], ia[2], ib[0], ib[1], ib[2], *om.triple))
            assert not _device_error, "an earlier call left a device error: %r" % _device_error
            ctx.enqueue_ssimh(ps, 1, 1.0, enc, sums.ptr, window=win)
            _sync(ctx)
            assert same64(sums.download(np.float64, (1,)), dense[0]), (fx, fy)
            ga, gb = (ssim_amd.GradH * 1)(ssim_amd.GradH(*oa.triple)), (ssim_amd.GradH * 1)(ssim_amd.GradH(*ob.triple))
            ctx.enqueue_ssimh_grad(ps, 1, 1.0, enc, go.ptr, ga, gb, window=win)
            ga, gb = (ssim_amd.GradH * 1)(ssim_amd.GradH(*pa.triple)), (ssim_amd.GradH * 1)(ssim_amd.GradH(*pb.triple))
            ctx.enqueue_ssimh_map_grad(ps, 1, 1.0, enc, (ssim_amd.GradOutF * 1)(ssim_amd.GradOutF(*ig)), ga, gb, window=win)
            _sync(ctx)
            done.append(((fx, fy), om, oa, ob, pa, pb))
        vol16.collect(full=True)                          # nothing but the output planes changed
        vol32.collect(full=True)
        for d, om, oa, ob, pa, pb in done:
            assert HM.same_f32(om.plane, dense[1][0]), d
            for o, want in ((oa, dense[2][0][0]), (ob, dense[2][0][1]), (pa, dense_map[2][0][0]), (pb, dense_map[2][0][1])):
                assert np.array_equal(o.plane, want), d
    finally:
        for v in (vol16, vol32, go, sums):
            if v is not None:
                v.free()


# ---- content -------------------------------------------------------------------------------------------------------------------------

@ENC
@WIN
@pytest.mark.parametrize("at", [(17, 20), (0, 0), (34, 0)], ids=["interior", "corner", "far-corner"])
def test_the_reach_of_a_nan_is_the_windows(device, window, enc, at):
    """40 x 35, one NaN at (row, column) `at`.  A NaN sample: exactly the (2R + 1)^2 map pixels and the (4R + 1)^2 gradient pixels around
    it, clipped; a NaN in gMap: (2R + 1)^2 gradient pixels -- not 11^2 / 21^2.  Everything else is finite, and every bit is the float32
    path's: exactly the pixels that path marks."""
    R = K.radius(window)
    w, h = 40, 35
    a, b = IN.random_pair(w, h, 11, enc)
    yy, xx = np.mgrid[0:h, 0:w]

    def box(reach):
        return (np.abs(yy - at[0]) <= reach) & (np.abs(xx - at[1]) <= reach)
    an = a.copy()
    an[at] = NAN16[enc]
    (_, ms, gr), _ = check_against_float32(device, enc, [(an, b)], 1.0, window, "NaN sample", g_out=[float(w * h)])
    assert np.array_equal(np.isnan(ms[0]), box(R)) and np.all(np.isfinite(ms[0][~box(R)]))
    for g in gr[0]:
        assert np.array_equal(HM.is_nan(g, enc), box(2 * R)) and np.all(np.isfinite(HM.widen(g, enc)[~box(2 * R)]))
    gm = np.full(a.shape, 0.01, np.float32)
    gm[at] = np.nan
    (_, _, gr), _ = check_against_float32(device, enc, [(a, b)], 1.0, window, "NaN in gMap", gmaps=[gm], maps=False)
    for g in gr[0]:
        assert np.array_equal(HM.is_nan(g, enc), box(R)) and np.all(np.isfinite(HM.widen(g, enc)[~box(R)]))


@ENC
@WIN
def test_subnormal_results_are_kept_and_overflow_gives_inf(device, window, enc):
    """The planes and the two upstream gradients of ssimhk_inputs, whose condition tests/test_ssimhk_cpu.py checks with the float64
    model: at G_SMALL the float16 gradients lie among the subnormals, which are kept, not flushed; at G_LARGE -- the scale arrives in the
    float32 upstream gradient, before the single rounding -- part of the pixels overflow to Inf and the others stay normal numbers.
    bfloat16 has float32's exponent range: its overflow is reached through one float of gMap."""
    pair = IN.rounding_pair(enc)
    (_, _, small), _ = check_against_float32(device, enc, [pair], 1.0, window, "G_SMALL", g_out=[IN.G_SMALL], maps=False)
    (_, _, large), (_, _, f32) = check_against_float32(device, enc, [pair], 1.0, window, "G_LARGE", g_out=[IN.G_LARGE], maps=False)
    for k, what in ((constant_k(IN.G_SMALL, pair[0].shape), "G_SMALL through gMap"), (constant_k(IN.G_LARGE, pair[0].shape), "G_LARGE through gMap")):
        (_, _, gr), _ = check_against_float32(device, enc, [pair], 1.0, window, what, gmaps=[k], maps=False)
        assert same_grads(gr[0], (small if "SMALL" in what else large)[0])
    for side in range(2):
        cs, cl = IN.census(small[0][side], enc), IN.census(large[0][side], enc)
        print("%s %s side %d (subnormal, Inf, normal): G_SMALL %r, G_LARGE %r" % (K.name_of(window), enc, side, cs, cl))
        if enc == HM.F16:
            assert cs[0] >= 100 and cs[1] == 0 and cl[1] >= 100 and cl[2] >= 100, (cs, cl)
        else:
            assert cs[0] == 0 and cl[1] == 0 and cl[2] > 0, (cs, cl)
    if enc == HM.BF16:
        top = max(float(np.abs(f).max()) for f in f32[0]) / float(constant_k(IN.G_LARGE, pair[0].shape))       # the largest |gradient| per unit of k
        k = np.float32(min(4.0 * MAX16[enc] / top, 1.0e38))
        (_, _, gr), _ = check_against_float32(device, enc, [pair], 1.0, window, "overflow through gMap", gmaps=[k], maps=False)
        for g in gr[0]:
            inf = (g & 0x7FFF) == INF16[enc]
            print("%s %s: %d of %d pixels overflow to Inf at k = %g" % (K.name_of(window), enc, int(inf.sum()), g.size, float(k)))
            assert inf.sum() < g.size and (inf.sum() > 0 or float(k) == 1.0e38), int(inf.sum())


# ---- scheduling ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window,enc", [((3, 0.0, "uniform"), HM.BF16), ((9, 1.5, "gaussian"), HM.F16)], ids=["3-box-bfloat16", "9-gaussian-float16"])
def test_tall_strips_have_the_bits_of_the_lone_launch(device, window, enc):
    """300 pairs of 9 x 603 in one launch: the planner gives a launch of that many pairs strips of many 8-row cells (parked leaves,
    flushes of eight, a short last cell of 3 rows), where every other launch of this module has one cell per strip.  Seven distinct
    pairs drawn in a seeded order; three pairs get a map.  Every pair has the bits of its lone launch -- sum, map, gradient and map
    gradient --, and the lone launch has the bits of the float32 windowed path."""
    w, h, n = 9, 603, 300
    pool = [IN.random_pair(w, h, 600 + i, enc) for i in range(7)]
    rng = np.random.default_rng(601)
    pick = [int(x) for x in rng.integers(0, 7, n)]
    pick[0], pick[n // 2], pick[-1] = 0, 3, 6
    gs = [float(w * h) * x for x in (-0.75, 0.5, 1.25)]
    gms = [(np.random.default_rng(610 + i).standard_normal((h, w)) * 100).astype(np.float32) for i in range(2)]
    lone, lone_g, lone_m = [], {}, {}
    for k, pair in enumerate(pool):
        (s, ms, _), _ = check_against_float32(device, enc, [pair], 1.0, window, ("lone", k))
        lone.append((s, ms[0]))
    assert len(set(s.tobytes() for s, _ in lone)) == 7
    for i in range(n):
        kg, km = (pick[i], i % 3), (pick[i], i % 2)
        if kg not in lone_g:
            lone_g[kg] = check_against_float32(device, enc, [pool[kg[0]]], 1.0, window, "lone gradient", g_out=[gs[kg[1]]], maps=False)[0][2][0]
        if km not in lone_m:
            lone_m[km] = check_against_float32(device, enc, [pool[km[0]]], 1.0, window, "lone map gradient", gmaps=[gms[km[1]]], maps=False)[0][2][0]
    pairs = [pool[k] for k in pick]
    s, _, gr = run(device, enc, pairs, 1.0, window, g_out=[gs[i % 3] for i in range(n)], maps=False)
    _, _, gm = run(device, enc, pairs, 1.0, window, gmaps=[gms[i % 2] for i in range(n)], maps=False)
    for i in range(n):
        assert same64(s[i:i + 1], lone[pick[i]][0]), i
        assert same_grads(gr[i], lone_g[(pick[i], i % 3)]) and same_grads(gm[i], lone_m[(pick[i], i % 2)]), i
    # the maps of the first, the middle and the last pair of the launch, the others none
    ctx = device.ctx
    bufs = [(ctx.upload(a), ctx.upload(b)) for a, b in pool]
    planes = [Plane(ctx, np.full((h, w), FILL32, np.float32), step=st, flip=fl, fill=FILL32) for st, fl in ((1, False), (3, False), (2, True))]
    sums = ctx.upload(np.full(n, -777.0))
    try:
        ps = (ssim_amd.Params16 * n)()
        where = {0: planes[0], n // 2: planes[1], n - 1: planes[2]}
        for i in range(n):
            da, db = bufs[pick[i]]
            m = where.get(i)
            ps[i] = ssim_amd.make_params16(w, h, da.ptr, 1, w, db.ptr, 1, w, *((m.ptr, m.dstep, m.dstride) if m else ()))
        entry(ctx, enc, "enqueue_ssim%s", window)(n, ps, 1.0, sums.ptr)
        _sync(ctx)
        device.sample()
        assert same64(sums.download(np.float64, (n,)), s)
        for i, m in where.items():
            assert HM.same_f32(m.read(), lone[pick[i]][1]), i
    finally:
        for x in [sums] + planes + [b for ab in bufs for b in ab]:
            x.free()


@ENC
@WIN
def test_alone_or_anywhere_in_a_batch_and_on_a_second_call(device, window, enc):
    """A batch of three different pairs and gOut values, in two orders, twice: each pair has the bits of its lone call."""
    w, h = 129, 17
    pairs = [IN.random_pair(w, h, 40 + i, enc) for i in range(3)]
    g = [x * w * h for x in (-0.75, 1.5, 0.25)]
    rng = np.random.default_rng(41)
    gms = [rng.standard_normal((h, w)).astype(np.float32) for _ in range(3)]
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
    """17 different pairs of 33 x 17: one forward and one gradient enqueue each, back to back -- 34 launches from the ring of 8 descriptor
    slots -- and one synchronise: the lone results."""
    ctx, (w, h), n = device.ctx, (33, 17), 17
    px, gap = w * h, 64
    win = mk(window)
    pairs = [IN.random_pair(w, h, 60 + i, enc) for i in range(n)]
    g_out = np.float32([(-0.75, 0.5, 1.0)[i % 3] * px for i in range(n)])
    lone = [run(device, enc, [pairs[i]], 1.0, window, g_out=[g_out[i]], maps=False) for i in range(n)]
    assert len(set(x[0].tobytes() for x in lone)) == n
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    bufs = [(ctx.upload(a), ctx.upload(b)) for a, b in pairs]
    per = px + gap
    fresh = np.full(2 * n * per + gap, FILL16, np.uint16)
    out, sums, go = ctx.upload(fresh), ctx.upload(np.full(n + 2, -777.0)), ctx.upload(g_out)
    try:
        keep = []
        for i in range(n):
            ps = (ssim_amd.Params16 * 1)(ssim_amd.make_params16(w, h, bufs[i][0].ptr, 1, w, bufs[i][1].ptr, 1, w))
            ga = (ssim_amd.GradH * 1)(ssim_amd.GradH(out.ptr + 2 * (gap + 2 * i * per), 1, w))
            gb = (ssim_amd.GradH * 1)(ssim_amd.GradH(out.ptr + 2 * (gap + (2 * i + 1) * per), 1, w))
            keep.append((ps, ga, gb))
            ctx.enqueue_ssimh(ps, 1, 1.0, enc, sums.ptr + 8 * (1 + i), window=win)
            ctx.enqueue_ssimh_grad(ps, 1, 1.0, enc, go.ptr + 4 * i, ga, gb, window=win)
        _sync(ctx)
        device.sample()
        s = sums.download(np.float64, (n + 2,))
        assert s[0] == -777.0 and s[-1] == -777.0
        host = out.download(np.uint16, fresh.shape)
        body = host[gap:].reshape(2 * n, per)
        assert np.all(host[:gap] == FILL16) and np.all(body[:, px:] == FILL16), "a gap between the gradient planes changed"
        for i in range(n):
            assert same64(s[1 + i:2 + i], lone[i][0]), i
            for side in range(2):
                assert np.array_equal(body[2 * i + side, :px].reshape(h, w), lone[i][2][0][side]), (i, side)
    finally:
        for x in [out, sums, go] + [b for ab in bufs for b in ab]:
            x.free()


@ENC
def test_windowed_16_bit_calls_share_one_context_with_the_other_families(device, enc):
    """On one context, 30 enqueues alternate without a host wait: forward, gradient and map gradient of 16-bit planes under five windows
    (every radius), interleaved with ssimf_win, ssimh, msssimh and ssim3h_win calls -- more than the 8 descriptor slots, all of them on
    the shared cell partials.  Every output has the bytes of the same call issued alone, with a host wait, on another context."""
    ctx = device.ctx
    sizes = [(129, 17), (33, 33)]
    data = []
    for i, (w, h) in enumerate(sizes):
        a, b = IN.random_pair(w, h, 200 + i, enc)
        k = (np.random.default_rng(210 + i).standard_normal((h, w)) * 100).astype(np.float32)
        data.append(dict(h=(ctx.upload(a), ctx.upload(b)), f=(ctx.upload(HM.widen(a, enc)), ctx.upload(HM.widen(b, enc))), k=ctx.upload(k),
                         go=ctx.upload(np.float32([(-0.75 + i) * w * h])), shape=(h, w)))
    va, vb = IN.random_pair(20 * 18, 13, 220, enc)             # a 20 x 18 x 13 volume for the ssim3h_win calls
    vol = dict(h=(ctx.upload(va), ctx.upload(vb)), shape=(13, 18, 20))
    kinds = []
    for j, win in enumerate(ONE_PER_RADIUS):
        kinds += [(0, "forward", "h", win), (1, "grad", "h", win), (0, "map_grad", "h", win),
                  (1, ("forward", "grad", "map_grad")[j % 3], "f", win), (j % 2, ("grad", "map_grad", "forward")[j % 3], "h", None),
                  (j % 2, "msssimh" if j % 2 else "ssim3h", "h", win)]
    assert len(kinds) == 30

    def issue(c, wait):
        outs, keep = [], []
        for shape_i, what, fam, _ in kinds:                 # the outputs first: an upload waits for its context's stream
            px = int(np.prod(vol["shape"] if what == "ssim3h" else data[shape_i]["shape"]))
            es = 4 if fam == "f" or what in ("forward", "ssim3h", "msssimh") else 2
            outs.append((ctx.upload(np.full(16, -777.0)), ctx.upload(np.full(px, -777.0, np.float32))) if es == 4 and what not in ("grad", "map_grad")
                        else (ctx.upload(np.zeros(px * es, np.uint8)), ctx.upload(np.zeros(px * es, np.uint8))))
        _sync(ctx)
        for (shape_i, what, fam, win), out in zip(kinds, outs):
            assert not _device_error, "an earlier call left a device error: %r" % _device_error
            item = data[shape_i]
            h, w = item["shape"]
            PS, GR, make = (ssim_amd.ParamsF, ssim_amd.GradF, ssim_amd.make_params_f) if fam == "f" else (ssim_amd.Params16, ssim_amd.GradH, ssim_amd.make_params16)
            pa, pb = item[fam]
            kw = {} if win is None else {"window": mk(win)}
            if what == "ssim3h":
                d3, h3, w3 = vol["shape"]
                ps = (ssim_amd.Params3H * 1)(ssim_amd.make_params3h(w3, h3, d3, vol["h"][0].ptr, (1, w3, w3 * h3), vol["h"][1].ptr, (1, w3, w3 * h3),
                                                                    out[1].ptr, (1, w3, w3 * h3)))
                c.enqueue_ssim3h(ps, 1, 1.0, enc, out[0].ptr, **kw)
            elif what == "msssimh":
                ps = (PS * 1)(make(w, h, pa.ptr, 1, w, pb.ptr, 1, w))
                c.enqueue_msssimh(ps, 1, 1.0, enc, out[0].ptr, out[0].ptr + 8, scales=3, weights=(0.3, 0.3, 0.4))
            elif what == "forward":
                ps = (PS * 1)(make(w, h, pa.ptr, 1, w, pb.ptr, 1, w, out[1].ptr, 1, w))
                head = (ps, 1, 1.0) if fam == "f" else (ps, 1, 1.0, enc)
                getattr(c, "enqueue_ssim" + fam)(*(head + (out[0].ptr,)), **kw)
            else:
                ps = (PS * 1)(make(w, h, pa.ptr, 1, w, pb.ptr, 1, w))
                head = (ps, 1, 1.0) if fam == "f" else (ps, 1, 1.0, enc)
                ga, gb = (GR * 1)(GR(out[0].ptr, 1, w)), (GR * 1)(GR(out[1].ptr, 1, w))
                keep.extend((ga, gb))
                if what == "grad":
                    getattr(c, "enqueue_ssim%s_grad" % fam)(*(head + (item["go"].ptr, ga, gb)), **kw)
                else:
                    ms = (ssim_amd.GradOutF * 1)(ssim_amd.GradOutF(item["k"].ptr, 1, w))
                    keep.append(ms)
                    getattr(c, "enqueue_ssim%s_map_grad" % fam)(*(head + (ms, ga, gb)), **kw)
            keep.append(ps)
            if wait:
                _sync(c)
        _sync(c)
        device.sample()
        got = []
        for out in outs:
            got.append(tuple(ctx.download(o.ptr, np.uint8, (o.nbytes,)).tobytes() for o in out))
            out[0].free()
            out[1].free()
        return got
    try:
        _sync(ctx)                                          # the uploads above, before another context's stream reads them
        with ssim_amd.Context(0) as other:
            alone = issue(other, True)
        mixed = issue(ctx, False)
        for i, kind in enumerate(kinds):
            assert mixed[i] == alone[i], (i, kind)
            assert any(alone[i][0]) and alone[i][0] != np.full(16, -777.0).tobytes(), (i, kind)
            if kind[1] != "msssimh":
                assert any(alone[i][1]) and alone[i][1] != np.full(len(alone[i][1]) // 4, -777.0, np.float32).tobytes(), (i, kind)
        assert alone[0][1] != alone[6][1] and alone[6][1] != alone[12][1]      # the windows differ: no call was compared with itself by accident
    finally:
        for item in data:
            for v in item["h"] + item["f"] + (item["k"], item["go"]):
                v.free()
        for v in vol["h"]:
            v.free()


# ---- PyTorch -------------------------------------------------------------------------------------------------------------------------
# torch brings its own HIP runtime; the checks run in ONE child process (tests/tools/ssimhk_torch_checks.py) that imports torch before
# the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    tool = os.path.join(ROOT, "tests", "tools", "ssimhk_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "ssimhk_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["value_and_gradient_are_the_c_abi_bit_for_bit", "non_contiguous_expanded_and_y_only", "a_scaled_loss_is_rounded_once",
                                   "side_stream", "default_keywords_are_ssim_bit_for_bit", "ssim_and_ssim_map_still_refuse_with_fixed_window"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
