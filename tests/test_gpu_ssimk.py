"""GPU: SSIM of float32 samples under a caller-chosen window (rmgr_ssim_hip_*_ssimf_win*, the window keyword of ssim_amd and
ssim_amd.torch_ops): held to the float64 definition (tests/ssimk_model.py) within bounds measured per window, to the entries without
_win bit for bit at the default window, and deterministic.

Bounds.  Measured, not estimated: ssimk_model.EMU holds, per window, what an fp32 emulation of the kernels' arithmetic leaves against the
float64 model over five golden pairs in two forms (tests/test_ssimk_cpu.py pins the figures); the bounds asserted here are twice those
(ssimk_model.tolerances): the project's standing margin for the 1-ulp reciprocal and the order of the fp64 sum.

Sizes are W x H.  1 x 1, 2 x 1, 1 x 2: the axis-of-one rule; 5 x 3, 4 x 4, 9 x 9: axes shorter than and equal to the window, both tails
overlapping; 33 x 33: a second gradient tile of one pixel and more than four 8-row strips; 129 x 17: a second strip column of one pixel;
7 x 300: many strips and tiles of a narrow column.  Every strip here holds one 8-row cell and no launch more than 3 pairs: strips of many
cells (9 x 603 and 9 x 2115 in 1000 pairs, 260 x 601 in 350) and gradient launches of 300 pairs are in tests/test_gpu_tall_strips.py.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sample_forms_inputs as IN
import ssimk_model as K
import ssim_amd
from conftest import ROOT
from test_gpu_ssimw import FILL32, Plane, random_pair, same

pytestmark = pytest.mark.gpu

G_OUT = -0.75
SIZES = ((1, 1), (2, 1), (1, 2), (5, 3), (4, 4), (9, 9), (33, 33), (129, 17), (7, 300))
BY_WINDOW = pytest.mark.parametrize("window", K.WINDOWS, ids=K.name_of)


def mk(window):
    """ssim_amd.Window of a ssimk_model window, or None."""
    if window is None:
        return None
    size, sigma, kind = window
    return ssim_amd.make_window(size, sigma if kind == "gaussian" else 1.5, kind)


def _wref(win):
    return None if win is None else ctypes.byref(win)


_device_error = []


def _ok(rc):
    """A library call's verdict.  Anything but success or a refused argument is a device error: nothing more is started on the GPU by
    this module after one."""
    if rc not in (0, 22):
        _device_error.append(rc)
    assert rc == 0, rc


def _sync(ctx):
    try:
        ctx.synchronize()
    except ssim_amd.SsimError as e:
        _device_error.append(e.errno)
        raise


def forward(ctx, pairs, r, win, want_map=True, step=1, flip=False, plain=False, entry="enqueue"):
    """The fp64 sums (entry "enqueue") or the float32 values ("device") and the maps of `pairs` under the Window `win` through the _win
    entry (win None: a NULL window); plain: through the entry without _win.  Every plane uses the layout (step, flip)."""
    n = len(pairs)
    h, w = pairs[0][0].shape
    made = []

    def plane(arr, **kw):
        made.append(Plane(ctx, arr, **kw))
        return made[-1]
    ps = (ssim_amd.ParamsF * n)()
    maps = []
    for i, (a, b) in enumerate(pairs):
        pa, pb = plane(np.asarray(a, np.float32), step=step, flip=flip), plane(np.asarray(b, np.float32), step=step, flip=flip)
        if want_map:
            m = plane(np.full((h, w), FILL32, np.float32), step=step, flip=flip, fill=FILL32)
            maps.append(m)
            ps[i] = ssim_amd.make_params_f(w, h, pa.ptr, pa.dstep, pa.dstride, pb.ptr, pb.dstep, pb.dstride, m.ptr, m.dstep, m.dstride)
        else:
            ps[i] = ssim_amd.make_params_f(w, h, pa.ptr, pa.dstep, pa.dstride, pb.ptr, pb.dstep, pb.dstride)
    lib = ctx.lib
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    if entry == "enqueue":
        sums = ctx.alloc(8 * n)
        rc = lib.rmgr_ssim_hip_enqueue_ssimf(ctx.handle, n, ps, r, sums.ptr) if plain else \
            lib.rmgr_ssim_hip_enqueue_ssimf_win(ctx.handle, n, ps, r, _wref(win), sums.ptr)
        _ok(rc)
        _sync(ctx)
        values = sums.download(np.float64, (n,))
        sums.free()
    else:
        out = (ctypes.c_float * n)()
        rc = lib.rmgr_ssim_hip_compute_ssimf_device(ctx.handle, n, ps, r, out) if plain else \
            lib.rmgr_ssim_hip_compute_ssimf_win_device(ctx.handle, n, ps, r, _wref(win), out)
        _ok(rc)
        values = np.array(out[:n], np.float32)
    got = [m.read() for m in maps]
    for p in made:
        p.free()
    return values, got


def backward(ctx, pairs, r, win, which=3, scalar=None, planes=None, stride0=None, step=1, flip=False, plain=False):
    """dLoss/dA and / or dLoss/dB of `pairs` under `win`: scalar = [gOut] through _ssimf_win_grad; planes = [gMap] or stride0 = [k] (one
    float per pair behind step = stride = 0) through _ssimf_win_map_grad; plain: the entries without _win.  Returns [(ga, gb)]."""
    n = len(pairs)
    h, w = pairs[0][0].shape
    made, bufs = [], []

    def plane(arr, **kw):
        made.append(Plane(ctx, arr, **kw))
        return made[-1]
    ps = (ssim_amd.ParamsF * n)()
    for i, (a, b) in enumerate(pairs):
        pa, pb = plane(np.asarray(a, np.float32), step=step, flip=flip), plane(np.asarray(b, np.float32), step=step, flip=flip)
        ps[i] = ssim_amd.make_params_f(w, h, pa.ptr, pa.dstep, pa.dstride, pb.ptr, pb.dstep, pb.dstride)
    arrs, outs = [None, None], [[], []]
    for k in range(2):
        if which & (1 << k):
            arrs[k] = (ssim_amd.GradF * n)()
            for i in range(n):
                g = plane(np.full((h, w), FILL32, np.float32), step=step, flip=flip, fill=FILL32)
                outs[k].append(g)
                arrs[k][i] = ssim_amd.GradF(g.ptr, g.dstep, g.dstride)
    lib = ctx.lib
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    if scalar is not None:
        go = ctx.upload(np.asarray(scalar, np.float32))
        bufs.append(go)
        rc = lib.rmgr_ssim_hip_enqueue_ssimf_grad(ctx.handle, n, ps, r, go.ptr, arrs[0], arrs[1]) if plain else \
            lib.rmgr_ssim_hip_enqueue_ssimf_win_grad(ctx.handle, n, ps, r, _wref(win), go.ptr, arrs[0], arrs[1])
    else:
        ms = (ssim_amd.GradOutF * n)()
        if stride0 is not None:
            go = ctx.upload(np.asarray(stride0, np.float32))
            bufs.append(go)
            for i in range(n):
                ms[i] = ssim_amd.GradOutF(go.ptr + 4 * i, 0, 0)
        else:
            for i in range(n):
                m = plane(np.asarray(planes[i], np.float32), step=step, flip=flip)
                ms[i] = ssim_amd.GradOutF(m.ptr, m.dstep, m.dstride)
        rc = lib.rmgr_ssim_hip_enqueue_ssimf_map_grad(ctx.handle, n, ps, r, ms, arrs[0], arrs[1]) if plain else \
            lib.rmgr_ssim_hip_enqueue_ssimf_win_map_grad(ctx.handle, n, ps, r, _wref(win), ms, arrs[0], arrs[1])
    _ok(rc)
    _sync(ctx)
    res = [tuple(outs[k][i].read() if arrs[k] is not None else None for k in range(2)) for i in range(n)]
    for p in made + bufs:
        p.free()
    return res


def same64(x, y):
    return np.array_equal(np.asarray(x, np.float64).view(np.uint64), np.asarray(y, np.float64).view(np.uint64))


def hold(ctx, window, a, b, r, what, ident=False):
    """Check 1 on one pair: value, map and both gradients for the scalar upstream gradient and the planes of ssimk_model.upstream_planes
    within the window's bounds.  Returns the worst figures."""
    px_tol, g_tol, grad_tol, ident_tol = K.tolerances(window)
    h, w = a.shape
    win = mk(window)
    sums, maps = forward(ctx, [(a, b)], r, win)
    want_v, want_m = K.ssim(a, b, r, window)
    e_px = float(np.abs(maps[0] - want_m).max())
    e_g = abs(float(sums[0]) / (float(w) * float(h)) - want_v)
    print("%s: per pixel %.3g (bound %.3g), global %.3g (bound %.3g)" % (what, e_px, px_tol, e_g, g_tol))
    assert np.all(np.isfinite(maps[0])) and e_px <= px_tol and e_g <= g_tol, (what, e_px, e_g)
    ups = list(K.upstream_planes(h, w))
    got = [backward(ctx, [(a, b)], r, win, scalar=[G_OUT])[0]] + backward(ctx, [(a, b)] * len(ups), r, win, planes=[p for _, p in ups])
    want = [K.grad(a, b, r, G_OUT, window)] + [K.grad_map(a, b, r, p, window) for _, p in ups]
    worst = 0.0
    for name, g, wt in zip(["scalar"] + [n for n, _ in ups], got, want):
        for side, gg, ww in (("dA", g[0], wt[0]), ("dB", g[1], wt[1])):
            assert np.all(np.isfinite(gg)), (what, name, side)
            if ident:
                if name == "scalar":
                    e = float(np.abs(gg).max()) * w * h * r / abs(G_OUT)
                    print("%s %s %s: exact gradient 0, max|grad| W H R = %.3g (bound %.3g)" % (what, name, side, e, ident_tol))
                    assert e <= ident_tol, (what, name, side, e)
                continue
            e = float(np.abs(gg - ww).max() / np.abs(ww).max())
            worst = max(worst, e)
            print("%s %s %s: %.3g of max|grad| (bound %.3g)" % (what, name, side, e, grad_tol))
            assert e <= grad_tol, (what, name, side, e)
    return e_px, e_g, worst


# ---- 1. the float64 model ----

@BY_WINDOW
def test_sizes_against_the_model(gpu_ctx, window):
    for w, h in SIZES:
        a, b = random_pair(w, h, 100 * w + h)
        hold(gpu_ctx, window, a, b, 1.0, "%s %dx%d" % (K.name_of(window), w, h))


@BY_WINDOW
def test_fixtures_in_two_forms_against_the_model(gpu_ctx, manifest, window):
    for name in K.FIXTURES:
        for form, fa, fb, r in K.fixture_forms(manifest, name):
            hold(gpu_ctx, window, fa, fb, r, "%s %s/%s" % (K.name_of(window), name, form))
        if name in ("bbb257x65_q50_ch1", "einstein_blur"):
            for form, fa, _, r in K.fixture_forms(manifest, name):
                hold(gpu_ctx, window, fa, fa, r, "%s %s/%s identical" % (K.name_of(window), name, form), ident=True)


# ---- 2. the default window has the bits of the entries without _win ----

@pytest.mark.parametrize("w,h", [(1, 1), (33, 33), (129, 17)])
def test_default_and_null_window_have_the_bits_of_the_entries_without_win(gpu_ctx, w, h):
    pairs = [random_pair(w, h, 7), random_pair(w, h, 8)]
    plane = [p for _, p in K.upstream_planes(h, w)]
    want_s, want_m = forward(gpu_ctx, pairs, 1.0, None, plain=True)
    want_v, _ = forward(gpu_ctx, pairs, 1.0, None, plain=True, entry="device")
    want_g = backward(gpu_ctx, pairs, 1.0, None, scalar=[G_OUT, 0.5], plain=True)
    want_p = backward(gpu_ctx, pairs, 1.0, None, planes=plane, plain=True)
    for win in (mk(K.DEFAULT), None):
        s, m = forward(gpu_ctx, pairs, 1.0, win)
        v, m2 = forward(gpu_ctx, pairs, 1.0, win, entry="device")
        assert same64(s, want_s) and same(v, want_v) and all(same(x, y) and same(z, y) for x, z, y in zip(m, m2, want_m))
        for got, want in ((backward(gpu_ctx, pairs, 1.0, win, scalar=[G_OUT, 0.5]), want_g), (backward(gpu_ctx, pairs, 1.0, win, planes=plane), want_p)):
            for g, wt in zip(got, want):
                assert same(g[0], wt[0]) and same(g[1], wt[1]) and np.abs(g[0]).max() > 0
        # the host entry and the Python keyword
        a, b = pairs[0]
        hv, hm = ssim_amd.compute_ssimf(a, b, 1.0, want_map=True, ctx=gpu_ctx, window=win)
        pv, pm = ssim_amd.compute_ssimf(a, b, 1.0, want_map=True, ctx=gpu_ctx)
        assert same(np.float32([hv]), np.float32([pv])) and same(hm, pm) and same(hm, want_m[0])
        # the host entry itself, with this window (NULL included)
        out, m = (ctypes.c_float * 1)(), np.empty((h, w), np.float32)
        ps = (ssim_amd.ParamsF * 1)(ssim_amd.make_params_f(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w, m.ctypes.data, 1, w))
        _ok(gpu_ctx.lib.rmgr_ssim_hip_compute_ssimf_win_host(gpu_ctx.handle, 1, ps, 1.0, _wref(win), out))
        assert same(np.float32([out[0]]), np.float32([pv])) and same(m, pm)


# ---- 3. batch and view invariance ----

@BY_WINDOW
def test_same_bits_alone_in_a_batch_through_views_and_with_one_gradient_or_both(gpu_ctx, window):
    w, h = 129, 17
    win = mk(window)
    pair = random_pair(w, h, 4)
    others = [random_pair(w, h, 5), random_pair(w, h, 6)]
    planes = [p for _, p in K.upstream_planes(h, w, seed=9)] + [next(K.upstream_planes(h, w, seed=10))[1]]
    s1, m1 = forward(gpu_ctx, [pair], 1.0, win)
    g1 = backward(gpu_ctx, [pair], 1.0, win, scalar=[G_OUT])[0]
    p1 = backward(gpu_ctx, [pair], 1.0, win, planes=[planes[0]])[0]
    assert np.abs(g1[0]).max() > 0 and np.abs(p1[1]).max() > 0
    for at in range(3):                                  # anywhere in a batch of three different pairs
        pairs, maps, gouts = list(others), [planes[1], planes[2]], [0.25, 2.0]
        pairs.insert(at, pair)
        maps.insert(at, planes[0])
        gouts.insert(at, G_OUT)
        s, m = forward(gpu_ctx, pairs, 1.0, win)
        assert same64(s[at], s1[0]) and same(m[at], m1[0]), at
        g = backward(gpu_ctx, pairs, 1.0, win, scalar=gouts)[at]
        p = backward(gpu_ctx, pairs, 1.0, win, planes=maps)[at]
        assert same(g[0], g1[0]) and same(g[1], g1[1]) and same(p[0], p1[0]) and same(p[1], p1[1]), at
    # samples, maps, upstream planes and gradient planes interleaved, stored back to front behind negative steps, and both; Plane.read
    # asserts that the gaps of a strided output plane still hold their fill
    for step, flip in ((3, False), (1, True), (2, True)):
        s, m = forward(gpu_ctx, [pair], 1.0, win, step=step, flip=flip)
        assert same64(s, s1) and same(m[0], m1[0]), (step, flip)
        g = backward(gpu_ctx, [pair], 1.0, win, scalar=[G_OUT], step=step, flip=flip)[0]
        p = backward(gpu_ctx, [pair], 1.0, win, planes=[planes[0]], step=step, flip=flip)[0]
        assert same(g[0], g1[0]) and same(g[1], g1[1]) and same(p[0], p1[0]) and same(p[1], p1[1]), (step, flip)
    for which in (1, 2):                                 # one gradient alone
        g = backward(gpu_ctx, [pair], 1.0, win, which=which, scalar=[G_OUT])[0]
        p = backward(gpu_ctx, [pair], 1.0, win, which=which, planes=[planes[0]])[0]
        assert g[2 - which] is None and p[2 - which] is None and same(g[which - 1], g1[which - 1]) and same(p[which - 1], p1[which - 1])
    s, m = forward(gpu_ctx, [pair], 1.0, win)            # a second call
    g = backward(gpu_ctx, [pair], 1.0, win, scalar=[G_OUT])[0]
    assert same64(s, s1) and same(m[0], m1[0]) and same(g[0], g1[0]) and same(g[1], g1[1])
    s, _ = forward(gpu_ctx, [pair], 1.0, win, want_map=False)
    assert same64(s, s1)                                 # with and without a map


# ---- 4. the identity clause ----

@BY_WINDOW
def test_constant_plane_and_stride_0_have_the_bits_of_the_scalar_gradient(gpu_ctx, window):
    win = mk(window)
    for w, h in ((1, 1), (5, 3), (33, 33), (129, 17)):
        pair = random_pair(w, h, 100 * w + h)
        k = K.constant_plane(G_OUT, h, w)
        assert k[0, 0] == np.float32(float(np.float32(G_OUT)) / (float(w) * float(h)))
        for which in (1, 2, 3):
            want = backward(gpu_ctx, [pair], 1.0, win, which, scalar=[G_OUT])[0]
            for got in (backward(gpu_ctx, [pair], 1.0, win, which, planes=[k])[0], backward(gpu_ctx, [pair], 1.0, win, which, stride0=[k[0, 0]])[0]):
                for g, wt in zip(got, want):
                    assert (g is None) == (wt is None)
                    if g is not None:
                        assert same(g, wt) and np.abs(g).max() > 0, (window, w, h, which)


# ---- 5. the reach of a NaN: what tells a radius-R kernel from a zero-padded 11-tap one ----

@BY_WINDOW
@pytest.mark.parametrize("at", [(20, 17), (0, 0), (39, 0)], ids=["interior", "corner", "far-corner"])
def test_nan_reach_is_the_radius(gpu_ctx, window, at):
    n, R = 40, K.radius(window)
    a, b = random_pair(n, n, 11)
    a = a.copy()
    a[at] = np.nan
    win = mk(window)
    _, maps = forward(gpu_ctx, [(a, b)], 1.0, win)
    ga, gb = backward(gpu_ctx, [(a, b)], 1.0, win, scalar=[1.0])[0]
    yy, xx = np.mgrid[0:n, 0:n]
    for name, got, reach in (("map", maps[0], R), ("dA", ga, 2 * R), ("dB", gb, 2 * R)):
        want = (np.abs(yy - at[0]) <= reach) & (np.abs(xx - at[1]) <= reach)
        assert np.array_equal(np.isnan(got), want), (window, at, name, int(np.isnan(got).sum()), int(want.sum()))
        assert np.all(np.isfinite(got[~want])), (window, at, name)
    # a NaN behind a per-pixel upstream gradient of zeros is still a NaN, over the same pixels
    pa, _ = backward(gpu_ctx, [(a, b)], 1.0, win, planes=[np.zeros((n, n), np.float32)])[0]
    assert np.array_equal(np.isnan(pa), (np.abs(yy - at[0]) <= 2 * R) & (np.abs(xx - at[1]) <= 2 * R)) and np.all(pa[~np.isnan(pa)] == 0)


# ---- 6. the 64-bit forms ----

@pytest.mark.parametrize("window", [(3, 0.0, "uniform"), (11, 2.0, "gaussian")], ids=K.name_of)
def test_64_bit_forms(gpu_ctx, window):
    """Samples, map, upstream plane and gradient planes 2^21 floats apart (fitsf_narrow() fails: the kernels' 64-bit lane offsets), read in
    either direction: the bits of the dense call, which meets the model."""
    from test_gpu_sample_forms import Volume
    ctx, win = gpu_ctx, mk(window)
    h, w = 12, 9
    a, b = IN.random_pair_f(h, w, np.random.default_rng(IN.SEED))
    gmap = next(K.upstream_planes(h, w, seed=3))[1]
    lay = IN.Layout(np.float32, IN.EDGE, w)
    for name, img in (("a", a), ("b", b), ("g", gmap)):
        lay.add(name, img)
    lay.close(out_rows=3 * 5 * h)
    vol = Volume(ctx, lay, np.float32(-3.0), FILL32)
    try:
        s0, m0 = forward(ctx, [(a, b)], 1.0, win)
        g0 = backward(ctx, [(a, b)], 1.0, win, scalar=[G_OUT])[0]
        p0 = backward(ctx, [(a, b)], 1.0, win, planes=[gmap])[0]
        px_tol, g_tol, grad_tol, _ = K.tolerances(window)
        want_v, want_m = K.ssim(a, b, 1.0, window)
        assert np.abs(m0[0] - want_m).max() <= px_tol and abs(float(s0[0]) / (w * h) - want_v) <= g_tol
        for got, want in ((g0, K.grad(a, b, 1.0, G_OUT, window)), (p0, K.grad_map(a, b, 1.0, gmap, window))):
            for g, wt in zip(got, want):
                assert np.abs(g - wt).max() <= grad_tol * np.abs(wt).max()
        go, sums = ctx.upload(np.float32([G_OUT])), ctx.alloc(8)
        done = []
        for fx, fy in ((False, False), (True, True), (True, False)):
            ia, ib, ig = vol.src("a", fx, fy), vol.src("b", fy, fx), vol.src("g", fx, fx)
            om, oa, ob, pa, pb = (vol.dst(h, w, f1, f2) for f1, f2 in ((fx, fy), (fy, fx), (fx, fx), (fy, fy), (not fx, fy)))
            ps = (ssim_amd.ParamsF * 1)(ssim_amd.make_params_f(w, h, ia[0], ia[1], ia[2], ib[0], ib[1], ib[2], *om.triple))
            ctx.enqueue_ssimf(ps, 1, 1.0, sums.ptr, window=win)
            ctx.synchronize()
            assert same64(sums.download(np.float64, (1,)), s0), (fx, fy)
            ga, gb = (ssim_amd.GradF * 1)(ssim_amd.GradF(*oa.triple)), (ssim_amd.GradF * 1)(ssim_amd.GradF(*ob.triple))
            ctx.enqueue_ssimf_grad(ps, 1, 1.0, go.ptr, ga, gb, window=win)
            ga, gb = (ssim_amd.GradF * 1)(ssim_amd.GradF(*pa.triple)), (ssim_amd.GradF * 1)(ssim_amd.GradF(*pb.triple))
            ctx.enqueue_ssimf_map_grad(ps, 1, 1.0, (ssim_amd.GradOutF * 1)(ssim_amd.GradOutF(*ig)), ga, gb, window=win)
            ctx.synchronize()
            done.append(((fx, fy), om, oa, ob, pa, pb))
        vol.collect(full=True)                            # nothing but the output planes changed
        for d, om, oa, ob, pa, pb in done:
            for o, want in ((om, m0[0]), (oa, g0[0]), (ob, g0[1]), (pa, p0[0]), (pb, p0[1])):
                assert same(o.plane, want), d
        go.free()
        sums.free()
    finally:
        vol.free()


# ---- 7. the host entry against the device entry ----

@BY_WINDOW
def test_host_entry_has_the_bits_of_the_device_entry(gpu_ctx, window):
    win = mk(window)
    for w, h in ((5, 3), (129, 17)):
        pairs = [random_pair(w, h, 21), random_pair(w, h, 22)]
        dv, dm = forward(gpu_ctx, pairs, 1.0, win, entry="device")
        for i, (a, b) in enumerate(pairs):
            hv, hm = ssim_amd.compute_ssimf(a, b, 1.0, want_map=True, ctx=gpu_ctx, window=win)
            assert same(np.float32([hv]), dv[i:i + 1]) and same(hm, dm[i])
            hv, _ = ssim_amd.compute_ssimf(a[::-1, ::-1], b[::-1, ::-1], 1.0, ctx=None, window=win)     # a default context, negative strides
            assert abs(float(hv) - float(dv[i])) <= 2 * K.tolerances(window)[1]
        assert same(ssim_amd.compute_ssimf_batch(pairs, 1.0, ctx=gpu_ctx, window=win), dv)
        assert same(gpu_ctx.ssimf_device(*_dense_params(gpu_ctx, pairs), 1.0, window=win), dv)


_kept = []


def _dense_params(ctx, pairs):
    """(ParamsF array, count) over dense device copies of `pairs`; the buffers live until the module ends."""
    ps = (ssim_amd.ParamsF * len(pairs))()
    for i, (a, b) in enumerate(pairs):
        da, db = ctx.upload(a), ctx.upload(b)
        _kept.extend((da, db))
        ps[i] = ssim_amd.make_params_f(a.shape[1], a.shape[0], da.ptr, 1, a.shape[1], db.ptr, 1, a.shape[1])
    return ps, len(pairs)


# ---- 8. torch ----
# torch brings a HIP runtime of its own, which has to be the first one a process loads: the checks run in one child process
# (tests/tools/ssimk_torch_checks.py) that imports torch before the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "ssimk_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "ssimk_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["forward_and_backward_are_the_c_abi_bit_for_bit", "slice_without_a_copy_and_a_side_stream",
                                   "gradient_agrees_with_the_conv2d_restatement", "default_arguments_are_todays_call_bit_for_bit"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
