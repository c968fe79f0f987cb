"""GPU: multi-scale SSIM of float32 volumes under a caller-chosen window and its gradient (rmgr_ssim_hip_enqueue_msssim3f_win,
rmgr_ssim_hip_compute_msssim3f_win_device / _host, rmgr_ssim_hip_enqueue_msssim3f_win_grad, ssim_amd.torch_ops.ms_ssim3d(win_size=...))
against the float64 definition (tests/msssim3k_model.py), and their determinism.  Sizes are W x H x D; arrays are (D, H, W).

Bounds.  Measured, not estimated, and fixed before the first GPU run: per window an fp32 emulation of the kernels' arithmetic
(msssim3k_model.Emulation) is measured against the float64 model on ssim3f_model.FIXTURES in two forms at Wang's 5 scales and at uniform
weights for 1, 3 and 8 scales (msssim3k_model.EMU; tests/test_msssim3k_cpu.py pins the figures); the bound is TOL_FACTOR (2.0) times the
figure.  The odd sizes have figures of their own, measured the same way on their own seeded inputs (msssim3k_model.ODD_EMU).  What the
MI355X itself left is written beside them in msssim3k_model.GPU.
"""
import ctypes
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import content_classes as C
import msssim3f_plan as MP
import msssim3k_inputs as IN
import msssim3k_model as MK
import ssim3f_chunks_inputs as CH
import ssim3f_model as S
import ssim3k_plan as PK
import ssim_amd
from conftest import ROOT
from test_gpu_ssim3f import LAYOUTS, SENT, Vol, random_pair, same
from test_gpu_ssim3k import mk
from test_gpu_ssim3k import run as run_single

pytestmark = pytest.mark.gpu

BY_WINDOW = pytest.mark.parametrize("window", MK.WINDOWS, ids=MK.name_of)
PER_RADIUS = [(3, 0.0, "uniform"), (5, 0.8, "gaussian"), (7, 0.0, "uniform"), (9, 1.5, "gaussian")]
BY_RADIUS = pytest.mark.parametrize("window", PER_RADIUS, ids=MK.name_of)
BOX3, G9 = IN.ODD_WINDOWS
ENGINE = (11, 1.5, "gaussian")
G_OUT = -0.75


def uniform(n):
    return (1.0 / n,) * n


@pytest.fixture(scope="module", autouse=True)
def module_report(gpu_ctx):
    """Prints what the module measured: seconds and the device memory in use before and after."""
    info0 = ssim_amd.memory_info(gpu_ctx)
    t0 = time.time()
    yield
    print("\nmsssim3k: %.1f s; memory_info before %r after %r" % (time.time() - t0, info0, ssim_amd.memory_info(gpu_ctx)))


def run(ctx, pairs, r, window, scales=5, weights=None, g_out=None, want=(True, True), lin="dense", lout="dense", inputs=None):
    """Forward (values, means) and -- g_out given -- backward of `pairs` under `window` (a model window; None: the entries without _win)
    in ONE enqueue each, device-resident.  Returns (values float64 (n,), means float64 (n, scales, 2), [(dA or None, dB or None)]).
    inputs: (Vol of A, Vol of B) per pair, uploaded by the caller."""
    win = mk(window)
    own = inputs is None
    if own:
        inputs = [(Vol(ctx, a.shape, lin, a), Vol(ctx, b.shape, lin, b)) for a, b in pairs]
    n = len(inputs)
    d, h, w = inputs[0][0].shape
    ps = (ssim_amd.Params3F * n)()
    for i, (va, vb) in enumerate(inputs):
        ps[i] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides)
    values, means = ctx.alloc(8 * n), ctx.alloc(16 * n * scales)
    ctx.enqueue_msssim3f(ps, n, r, values.ptr, means.ptr, scales, weights, window=win)
    gvols = [[], []]
    if g_out is not None:
        go = ctx.upload(np.asarray(g_out, np.float32).reshape(n))
        arrs = [None, None]
        for k in range(2):
            if want[k]:
                arrs[k] = (ssim_amd.Grad3F * n)()
                for i in range(n):
                    gv = Vol(ctx, (d, h, w), lout)
                    gvols[k].append(gv)
                    arrs[k][i] = ssim_amd.Grad3F(gv.ptr, *gv.strides)
        ctx.enqueue_msssim3f_grad(ps, n, r, means.ptr, go.ptr, arrs[0], arrs[1], scales, weights, window=win)
    ctx.synchronize()
    v, m = values.download(np.float64, (n,)), means.download(np.float64, (n, scales, 2))
    grads = [(gvols[0][i].result() if want[0] else None, gvols[1][i].result() if want[1] else None) for i in range(n)] if g_out is not None else []
    for x in gvols[0] + gvols[1] + ([go] if g_out is not None else []) + [values, means]:
        x.free()
    if own:
        for va, vb in inputs:
            va.free()
            vb.free()
    return v, m, grads


def same_result(x, y):
    """Values, means and every gradient of two run() results, bit for bit."""
    if not (same(x[0], y[0]) and same(x[1], y[1]) and len(x[2]) == len(y[2])):
        return False
    return all((p is None and q is None) or same(p, q) for gx, gy in zip(x[2], y[2]) for p, q in zip(gx, gy))


# ---- 1. against the float64 model ----

@BY_WINDOW
def test_golden_volumes_in_two_forms_at_wangs_scales(gpu_ctx, manifest, window):
    """The seven windows (the 11-tap box and 11 Gaussian 2 run the kernels of msssim3f_kernels.hip with other taps) on the five golden
    volumes in two forms at Wang's scales: value, every per-scale mean, both gradients, and the pair of identical volumes."""
    tv, tm, tg, ti = MK.tolerances(window)
    wv = wm = wg = wi = 0.0
    for name in S.FIXTURES:
        for form, fa, fb, r in S.fixture_forms(manifest, name):
            mod = MK.Model(fa, fb, r, window)
            v, means, grads = run(gpu_ctx, [(fa, fb)], r, window, 5, None, [G_OUT])
            assert all(np.all(np.isfinite(g)) for g in grads[0])
            fv, fm, fg = MK.figures(v[0], means[0], grads[0], mod, 5, None, G_OUT)
            _, _, ident = run(gpu_ctx, [(fa, fa)], r, window, 5, None, [G_OUT])
            fi = MK.ident_figure(ident[0], fa.shape, r, G_OUT)
            print("%s %s/%s: value %.3g mean %.3g grad %.3g identical %.3g" % (MK.name_of(window), name, form, fv, fm, fg, fi))
            wv, wm, wg, wi = max(wv, fv), max(wm, fm), max(wg, fg), max(wi, fi)
    print("GPU %r: (%.3e, %.3e, %.3e, %.3e)" % (window, wv, wm, wg, wi))
    assert wv <= tv and wm <= tm and wg <= tg and wi <= ti, (window, (wv, wm, wg, wi), (tv, tm, tg, ti))


@BY_WINDOW
def test_one_golden_volume_at_one_three_and_eight_scales_and_a_zero_weight(gpu_ctx, manifest, window):
    tv, tm, tg, ti = MK.tolerances(window)
    _, a, b, r = S.fixture_forms(manifest, "bbb257x65_q50_ch1")[0]
    mod = MK.Model(a, b, r, window)
    worst = [0.0, 0.0, 0.0, 0.0]
    for scales, w in MK.CONFIGS[1:] + ((5, (0.25, 0.25, 0.0, 0.25, 0.25)),):
        v, means, grads = run(gpu_ctx, [(a, b)], r, window, scales, w, [G_OUT])
        fv, fm, fg = MK.figures(v[0], means[0], grads[0], mod, scales, w, G_OUT)
        _, _, ident = run(gpu_ctx, [(a, a)], r, window, scales, w, [G_OUT])
        fi = MK.ident_figure(ident[0], a.shape, r, G_OUT)
        print("%s, %d scales: value %.3g mean %.3g grad %.3g identical %.3g" % (MK.name_of(window), scales, fv, fm, fg, fi))
        worst = [max(x, y) for x, y in zip(worst, (fv, fm, fg, fi))]
    print("GPU %r at 1, 3, 8 scales and a zero weight: (%.3e, %.3e, %.3e, %.3e)" % ((window,) + tuple(worst)))
    assert worst[0] <= tv and worst[1] <= tm and worst[2] <= tg and worst[3] <= ti, (window, worst, (tv, tm, tg, ti))


@pytest.mark.parametrize("window", IN.ODD_WINDOWS, ids=MK.name_of)
def test_odd_sizes_whose_volumes_are_smaller_than_the_window(gpu_ctx, window):
    """The eight seeded odd sizes at 8 uniform scales: coarse volumes clamp under the window, down to 1 x 1 x 1; a gradient has the same
    bits alone and together with the other."""
    tv, tm, tg = MK.odd_tolerances(window)
    wts = uniform(IN.ODD_SCALES)
    wv = wm = wg = 0.0
    for (w, h, d), a, b, r in IN.odd_cases():
        mod = MK.Model(a, b, r, window)
        res = run(gpu_ctx, [(a, b)], r, window, IN.ODD_SCALES, wts, [G_OUT])
        v, means, grads = res
        assert all(g.shape == (d, h, w) and np.all(np.isfinite(g)) for g in grads[0])
        only_a = run(gpu_ctx, [(a, b)], r, window, IN.ODD_SCALES, wts, [G_OUT], want=(True, False))[2]
        only_b = run(gpu_ctx, [(a, b)], r, window, IN.ODD_SCALES, wts, [G_OUT], want=(False, True))[2]
        assert same(only_a[0][0], grads[0][0]) and same(only_b[0][1], grads[0][1]), (w, h, d)
        fv, fm, fg = MK.figures(v[0], means[0], grads[0], mod, IN.ODD_SCALES, wts, G_OUT)
        print("%s %dx%dx%d: value %.3g mean %.3g grad %.3g" % (MK.name_of(window), w, h, d, fv, fm, fg))
        wv, wm, wg = max(wv, fv), max(wm, fm), max(wg, fg)
    print("GPU odd %r: (%.3e, %.3e, %.3e)" % (window, wv, wm, wg))
    assert wv <= tv and wm <= tm and wg <= tg, (window, (wv, wm, wg), (tv, tm, tg))


# ---- 2. the default window is msssim3f ----

def test_null_and_the_engines_window_give_the_bits_of_msssim3f(gpu_ctx):
    ctx, lib = gpu_ctx, gpu_ctx.lib
    pairs = [random_pair((33, 20, 13), 5), random_pair((33, 20, 13), 6)]
    d, h, w = pairs[0][0].shape
    for scales, wts in ((5, None), (3, (0.2, 0.3, 0.5)), (1, (1.0,))):
        base = run(ctx, pairs, 1.0, None, scales, wts, [G_OUT, 0.5])
        assert same_result(run(ctx, pairs, 1.0, ENGINE, scales, wts, [G_OUT, 0.5]), base)
        h0 = ssim_amd.compute_msssim3f_batch(pairs, 1.0, scales, wts, per_scale=True)
        h1 = ssim_amd.compute_msssim3f_batch(pairs, 1.0, scales, wts, per_scale=True, window=mk(ENGINE))
        assert same(h1[0], h0[0]) and same(h1[1], h0[1]) and same(h0[1], base[1]) and same(h0[0], base[0].astype(np.float32))
        # a NULL window through the _win entries themselves (the binding's window=None calls the entries without _win)
        vols = [(Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b)) for a, b in pairs]
        ps = (ssim_amd.Params3F * 2)()
        for i, (va, vb) in enumerate(vols):
            ps[i] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides)
        d1 = ctx.msssim3f_device(ps, 2, 1.0, scales, wts, per_scale=True, window=mk(ENGINE))
        assert same(d1[0], h0[0]) and same(d1[1], h0[1])
        cw = None if wts is None else (ctypes.c_double * scales)(*wts)
        vals, means, go = ctx.alloc(16), ctx.alloc(32 * scales), ctx.upload(np.float32([G_OUT, 0.5]))
        gv = [[Vol(ctx, (d, h, w)) for _ in range(2)] for _ in range(2)]
        arrs = [(ssim_amd.Grad3F * 2)(), (ssim_amd.Grad3F * 2)()]
        for k in range(2):
            for i in range(2):
                arrs[k][i] = ssim_amd.Grad3F(gv[k][i].ptr, *gv[k][i].strides)
        assert lib.rmgr_ssim_hip_enqueue_msssim3f_win(ctx.handle, 2, ps, 1.0, None, scales, cw, vals.ptr, means.ptr) == 0
        assert lib.rmgr_ssim_hip_enqueue_msssim3f_win_grad(ctx.handle, 2, ps, 1.0, None, scales, cw, means.ptr, go.ptr, arrs[0], arrs[1]) == 0
        ctx.synchronize()
        assert same(vals.download(np.float64, (2,)), base[0]) and same(means.download(np.float64, (2, scales, 2)), base[1])
        for i in range(2):
            assert same(gv[0][i].result(), base[2][i][0]) and same(gv[1][i].result(), base[2][i][1])
        out = (ctypes.c_float * 2)()
        hm = (ctypes.c_double * (4 * scales))()
        assert lib.rmgr_ssim_hip_compute_msssim3f_win_device(ctx.handle, 2, ps, 1.0, None, scales, cw, out, hm) == 0
        assert same(np.array(out[:], np.float32), h0[0]) and same(np.array(hm[:], np.float64).reshape(2, scales, 2), h0[1])
        hp = (ssim_amd.Params3F * 2)()
        for i, (a, b) in enumerate(pairs):
            hp[i] = ssim_amd.make_params3f(w, h, d, a.ctypes.data, (1, w, w * h), b.ctypes.data, (1, w, w * h))
        assert lib.rmgr_ssim_hip_compute_msssim3f_win_host(None, 2, hp, 1.0, None, scales, cw, out, hm) == 0
        assert same(np.array(out[:], np.float32), h0[0]) and same(np.array(hm[:], np.float64).reshape(2, scales, 2), h0[1])
        for x in [vals, means, go] + gv[0] + gv[1] + [v for p in vols for v in p]:
            x.free()


# ---- 3. bit identities with the single-scale family ----

@BY_RADIUS
def test_mssim_of_every_scale_is_ssim3f_win_on_the_pyramid(gpu_ctx, window):
    a, b = random_pair((37, 21, 44), 11)
    _, m, _ = run(gpu_ctx, [(a, b)], 1.0, window, 8, uniform(8))
    pa, pb = MK.pyramid(a, 8, np.float32), MK.pyramid(b, 8, np.float32)
    for s in range(8):
        assert pa[s].dtype == np.float32
        sums, _, _ = run_single(gpu_ctx, [(pa[s], pb[s])], 1.0, window, maps=False)
        assert same(np.float64([sums[0] / S.voxels(pa[s].shape)]), m[0, s, 1:2]), s


@BY_RADIUS
def test_one_scale_is_the_windowed_map_gradient_under_a_constant(gpu_ctx, window):
    a, b = random_pair((33, 20, 13), 12)
    d, h, w = a.shape
    g_out = np.float32(G_OUT)
    v, m, grads = run(gpu_ctx, [(a, b)], 1.0, window, 1, (1.0,), [g_out])
    ms = float(m[0, 0, 1]) ** 1.0
    assert same(np.float64([ms]), v)
    k0 = np.float32((((float(g_out) * 1.0) * ms) / float(m[0, 0, 1])) / (float(w) * float(h) * float(d)))
    _, _, want = run_single(gpu_ctx, [(a, b)], 1.0, window, ks=[k0], scalar_k=True, forward=False)
    assert same(want[0][0], grads[0][0]) and same(want[0][1], grads[0][1]) and np.abs(grads[0][0]).max() > 0


# ---- 4. determinism ----

@pytest.mark.parametrize("window", [BOX3, (7, 1.5, "gaussian")], ids=MK.name_of)
def test_seven_pairs_in_one_call_and_the_same_call_twice(gpu_ctx, window):
    size = (33, 20, 13)
    pairs = [random_pair(size, 40 + i) for i in range(7)]
    g = [-0.75, 1.5, 0.25, 1.0, -2.0, 0.5, 3.0]
    alone = [run(gpu_ctx, [pairs[i]], 1.0, window, 4, uniform(4), [g[i]]) for i in range(7)]
    for call in range(2):
        v, m, gr = run(gpu_ctx, pairs, 1.0, window, 4, uniform(4), g)
        for i in range(7):
            assert same(v[i:i + 1], alone[i][0]) and same(m[i], alone[i][1][0]), (i, call)
            assert same(gr[i][0], alone[i][2][0][0]) and same(gr[i][1], alone[i][2][0][1]), (i, call)
    for k, want in ((0, (True, False)), (1, (False, True))):
        _, _, gr = run(gpu_ctx, pairs, 1.0, window, 4, uniform(4), g, want=want)
        for i in range(7):
            assert gr[i][1 - k] is None and same(gr[i][k], alone[i][2][0][k]), (i, k)


@pytest.mark.parametrize("window", [BOX3, G9], ids=MK.name_of)
@pytest.mark.parametrize("size,scales", [((17, 17, 131), 3), ((5, 3, 1000), 4)], ids=lambda s: str(s))
def test_chunk_depths_of_every_scale_change_no_bit(gpu_ctx, size, scales, window):
    """Launches of 1 and of 40 volumes: under the 9-tap window plan3k picks other chunk depths at scale 0 (asserted through
    tests/ssim3k_plan.py); under the 3-tap box, whose chunks pay two warm-up slices, it mostly keeps the shallowest -- the depths are
    printed.  The 40 are drawn from seven distinct pairs and five dLoss/dS values (ssim3f_chunks_inputs.picks: neighbours differ): every
    value, mean and gradient has the bits of ITS OWN (pair, dLoss/dS) combination launched alone."""
    n = 40
    radius = MK.radius(window)
    cus = int(re.search(r"(\d+) CUs", gpu_ctx.describe()).group(1))
    depths = {k: [PK.plan3k(radius, *(MP.dims(*size, s) + (k, cus))).chunk_slices for s in range(scales)] for k in (1, n)}
    print("chunk depths per scale on %d CUs at radius %d: %r" % (cus, radius, depths))
    assert radius != 4 or depths[1][0] != depths[n][0], depths
    pairs = CH.pairs(size)
    which, g_of = CH.picks(n, 3)
    combos = list(zip(which.tolist(), g_of.tolist()))
    vols = [(Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)) for a, b in pairs]
    lone = {c: run(gpu_ctx, None, 1.0, window, scales, uniform(scales), [CH.G_OUTS[c[1]]], inputs=[vols[c[0]]]) for c in sorted(set(combos))}
    v, m, gr = run(gpu_ctx, None, 1.0, window, scales, uniform(scales), [CH.G_OUTS[c[1]] for c in combos], inputs=[vols[c[0]] for c in combos])
    for i, c in enumerate(combos):
        assert same(v[i:i + 1], lone[c][0]) and same(m[i], lone[c][1][0]), (i, c)
        assert same(gr[i][0], lone[c][2][0][0]) and same(gr[i][1], lone[c][2][0][1]), (i, c)
    assert np.abs(gr[0][0]).max() > 0
    for va, vb in vols:
        va.free()
        vb.free()


@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "dense"])
def test_views_give_the_bits_of_the_dense_volume(gpu_ctx, layout):
    a, b = random_pair((37, 19, 14), 77)
    for window in (BOX3, G9):
        dense = run(gpu_ctx, [(a, b)], 1.0, window, 3, uniform(3), [G_OUT])
        for lin, lout in ((layout, layout), (layout, "dense"), ("dense", layout)):
            assert same_result(run(gpu_ctx, [(a, b)], 1.0, window, 3, uniform(3), [G_OUT], lin=lin, lout=lout), dense), (window, lin, lout)


def test_device_host_and_enqueue_entries_agree(gpu_ctx):
    a, b = random_pair((37, 19, 14), 78)
    for window in (BOX3, (7, 0.0, "uniform")):
        win = mk(window)
        v, m, _ = run(gpu_ctx, [(a, b)], 1.0, window)
        want = np.float32(v[0])
        for ctx in (None, gpu_ctx):
            hv, hm = ssim_amd.compute_msssim3f(a, b, 1.0, per_scale=True, ctx=ctx, window=win)
            assert same(np.float32([hv]), np.float32([want])) and same(hm, m[0])
        ta, tb = np.ascontiguousarray(a.transpose(1, 2, 0)[::-1]), np.ascontiguousarray(b[:, :, ::-1])
        hv = ssim_amd.compute_msssim3f(ta[::-1].transpose(2, 0, 1), tb[:, :, ::-1], 1.0, window=win)      # permuted and negative-step host views
        assert same(np.float32([hv]), np.float32([want]))
        vs, ms = ssim_amd.compute_msssim3f_batch([(a, b), (b, a), (a, a)], 1.0, per_scale=True, window=win)
        assert same(vs[:1], np.float32([want])) and same(ms[0], m[0]) and abs(float(vs[2]) - 1.0) < 1e-6
        va, vb = Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)
        ps = (ssim_amd.Params3F * 1)()
        ps[0] = ssim_amd.make_params3f(37, 19, 14, va.ptr, va.strides, vb.ptr, vb.strides)
        dv, dm = gpu_ctx.msssim3f_device(ps, 1, 1.0, per_scale=True, window=win)
        assert same(dv, np.float32([want])) and same(dm, m)
        va.free()
        vb.free()


# ---- 5. slices far apart ----

@BY_RADIUS
@pytest.mark.parametrize("sign", [1, -1], ids=["forwards", "backwards"])
def test_slices_two_to_the_21_floats_apart(gpu_ctx, window, sign):
    """One 9 x 5 x 3 pair at 2 scales whose slices lie 2^21 floats apart -- A, B and both gradients, each at its own place in one device
    buffer --, ascending and descending: the bits of the dense call, and nothing but the gradient volumes written."""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    w, h, d, far = 9, 5, 3, 1 << 21
    a, b = random_pair((w, h, d), 33)
    scales, wts, win = 2, (0.4, 0.6), mk(window)
    dense = run(ctx, [(a, b)], 1.0, window, scales, wts, [45.0])
    room = 64                                                     # floats per item and slice (>= w * h)
    total = 2 * far + 4 * room
    host = np.full(total, SENT, np.float32)
    z0 = 0 if sign == 1 else d - 1

    def at(item, z):
        return z * far + item * room
    for item, vol in ((0, a[::sign]), (1, b[::sign])):
        for z in range(d):
            host[at(item, z):at(item, z) + w * h] = vol[z].reshape(-1)
    buf = ctx.upload(host)
    strides = (1, w, sign * far)
    ps = (ssim_amd.Params3F * 1)()
    ps[0] = ssim_amd.make_params3f(w, h, d, buf.ptr + 4 * at(0, z0), strides, buf.ptr + 4 * at(1, z0), strides)
    ga, gb = (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)()
    ga[0], gb[0] = ssim_amd.Grad3F(buf.ptr + 4 * at(2, z0), *strides), ssim_amd.Grad3F(buf.ptr + 4 * at(3, z0), *strides)
    vals, means, go = ctx.alloc(8), ctx.alloc(16 * scales), ctx.upload(np.float32([45.0]))
    ctx.enqueue_msssim3f(ps, 1, 1.0, vals.ptr, means.ptr, scales, wts, window=win)
    ctx.enqueue_msssim3f_grad(ps, 1, 1.0, means.ptr, go.ptr, ga, gb, scales, wts, window=win)
    ctx.synchronize()
    assert same(vals.download(np.float64, (1,)), dense[0]) and same(means.download(np.float64, (1, scales, 2)), dense[1])
    got = buf.download(np.float32, (total,))
    for item, want in ((2, dense[2][0][0]), (3, dense[2][0][1])):
        vol = np.stack([got[at(item, z):at(item, z) + w * h].reshape(h, w) for z in range(d)])[::sign]
        assert same(np.ascontiguousarray(vol), want), (item, sign)
        for z in range(d):
            got[at(item, z):at(item, z) + w * h] = host[at(item, z):at(item, z) + w * h]
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32)), "a float outside the gradient volumes was written"
    for x in (buf, vals, means, go):
        x.free()


# ---- 6. sub-batches and the context's scratch ----

def test_sub_batches_of_the_forward_and_of_the_backward(gpu_ctx):
    """One more volume of 96^3 at two scales than a sub-batch of the backward for both gradients holds (tests/msssim3f_plan.py: the
    scratch does not depend on the window): two sub-batches, under the 3-tap box.  The forward of one more volume of 2 x 1 x 3 than its
    launch limit holds: sub-batches of 65535 and of one.  The volumes around each boundary differ from their neighbours; every value, mean
    and gradient has the bits of its own combination launched alone."""
    size, scales = (96, 96, 96), 2
    n = MP.per_sub_batch(*size, scales, 2) + 1
    assert n == 68 and MP.sub_batches(*size, scales, 2, n) == [(0, 67), (67, 1)]
    pairs = [random_pair(size, 3 + k) for k in range(3)]
    g_outs = CH.G_OUTS[:3]
    which, g_of = CH.picks(n, 5)
    combos = [(k % len(pairs), g % len(g_outs)) for k, g in zip(which.tolist(), g_of.tolist())]
    for i in (65, 66):
        assert combos[i][0] != combos[i + 1][0] and combos[i][1] != combos[i + 1][1], combos[65:]
    vols = [(Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)) for a, b in pairs]
    lone = {c: run(gpu_ctx, None, 1.0, BOX3, scales, uniform(scales), [g_outs[c[1]]], inputs=[vols[c[0]]]) for c in sorted(set(combos))}
    for c in lone:
        assert np.abs(lone[c][2][0][0]).max() > 0 and np.abs(lone[c][2][0][1]).max() > 0
    v, m, gr = run(gpu_ctx, None, 1.0, BOX3, scales, uniform(scales), [g_outs[c[1]] for c in combos], inputs=[vols[c[0]] for c in combos])
    for i, c in enumerate(combos):
        assert same(v[i:i + 1], lone[c][0]) and same(m[i], lone[c][1][0]), (i, c)
        assert same(gr[i][0], lone[c][2][0][0]) and same(gr[i][1], lone[c][2][0][1]), (i, c)
    for va, vb in vols:
        va.free()
        vb.free()
    # the forward
    size = (2, 1, 3)
    n = MP.per_sub_batch(*size, scales, 0) + 1
    assert n == 65536 and MP.sub_batches(*size, scales, 0, n) == [(0, 65535), (65535, 1)]
    pairs = [random_pair(size, 90 + k) for k in range(5)]
    which = np.random.default_rng([CH.SEED, n]).permutation(np.arange(n) % len(pairs)).tolist()
    assert which[n - 1] != which[n - 2] and which[n - 1] != which[0]
    vols = [(Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)) for a, b in pairs]
    lone = [run(gpu_ctx, None, 1.0, BOX3, scales, uniform(scales), inputs=[vols[k]]) for k in range(len(pairs))]
    v, m, _ = run(gpu_ctx, None, 1.0, BOX3, scales, uniform(scales), inputs=[vols[k] for k in which])
    pick = np.asarray(which)
    bad = np.flatnonzero((v.view(np.uint64) != np.concatenate([lone[k][0] for k in range(len(pairs))])[pick].view(np.uint64)) |
                         np.any(m.view(np.uint64) != np.concatenate([lone[k][1] for k in range(len(pairs))])[pick].view(np.uint64), axis=(1, 2)))
    assert len(bad) == 0, "%d of %d volumes differ from their pair launched alone; the first: volume %d" % (len(bad), n, bad[0])
    for va, vb in vols:
        va.free()
        vb.free()


def test_a_default_window_forward_between_a_windowed_forward_and_its_backward(gpu_ctx):
    """The windowed forward, a default-window forward of another shape on the same context (it overwrites the pyramid and the partials),
    then the windowed backward: the backward recomputes its pyramid, so the gradient has the bits of the undisturbed sequence."""
    ctx = gpu_ctx
    window = (7, 1.5, "gaussian")
    win = mk(window)
    a, b = random_pair((40, 36, 20), 21)
    other = random_pair((21, 50, 33), 22)
    want = run(ctx, [(a, b)], 1.0, window, 5, None, [G_OUT])
    d, h, w = a.shape
    va, vb = Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b)
    ps = (ssim_amd.Params3F * 1)()
    ps[0] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides)
    vals, means, go = ctx.alloc(8), ctx.alloc(80), ctx.upload(np.float32([G_OUT]))
    ctx.enqueue_msssim3f(ps, 1, 1.0, vals.ptr, means.ptr, window=win)
    ov, _, _ = run(ctx, [other, other], 1.0, None)
    assert np.all(np.isfinite(ov))
    ga, gb = Vol(ctx, a.shape), Vol(ctx, a.shape)
    pa, pb = (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)()
    pa[0], pb[0] = ssim_amd.Grad3F(ga.ptr, *ga.strides), ssim_amd.Grad3F(gb.ptr, *gb.strides)
    ctx.enqueue_msssim3f_grad(ps, 1, 1.0, means.ptr, go.ptr, pa, pb, window=win)
    ctx.synchronize()
    assert same(vals.download(np.float64, (1,)), want[0]) and same(ga.result(), want[2][0][0]) and same(gb.result(), want[2][0][1])
    for x in (va, vb, ga, gb, vals, means, go):
        x.free()


# ---- 7. NaN, a zero upstream gradient and the ReLU ----

@pytest.mark.parametrize("window", [BOX3, G9, (11, 0.0, "uniform")], ids=MK.name_of)
def test_nan_sample_a_zero_upstream_gradient_and_the_relu_pair(gpu_ctx, window):
    a, b = random_pair((33, 20, 13), 5)
    x = a.copy()
    x[6, 10, 16] = np.nan
    v, _, _ = run(gpu_ctx, [(x, b)], 1.0, window, 3, uniform(3))
    assert np.isnan(v[0])
    # gOut = 0: every gradient voxel +0, even with a NaN sample
    for vol in (a, x):
        _, _, gr = run(gpu_ctx, [(vol, b)], 1.0, window, 3, uniform(3), [0.0])
        for g in gr[0]:
            assert not np.any(g.view(np.uint32)), "a gradient voxel is not +0"
    # the anticorrelated pair: the product is clamped to 0, the gradient is +0 everywhere, its batch neighbour is untouched by it
    _, ca, cb, r, _ = C.named([c for c in C.volume_classes((12, 19, 40), 1.0) if c[0] not in C.HUGE_CLASSES], "anticorrelated")
    assert MK.Model(ca, cb, r, window).means(4)[0][0] < 0
    v, m, gr = run(gpu_ctx, [(ca, cb), (ca, ca)], r, window, 4, uniform(4), [1.0, 1.0])
    assert m[0][0][0] < 0 and v[0] == 0.0 and abs(v[1] - 1.0) < 1e-5
    for g in gr[0]:
        assert not np.any(g.view(np.uint32)), "a gradient voxel is not +0"
    assert all(np.all(np.isfinite(g)) for g in gr[1])


# ---- torch ----
# torch brings a HIP runtime of its own, which has to be the first one a process loads: the checks run in one child process
# (tests/tools/msssim3k_torch_checks.py) that imports torch before the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "msssim3k_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "msssim3k_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["windowed_ms_ssim3d_is_the_c_abi_bit_for_bit", "windowed_ms_ssim3d_amp_on_16_bit_tensors_is_the_c_abi_bit_for_bit",
                                   "loss_under_autocast_hands_out_a_bfloat16_gradient", "default_keywords_give_the_bits_of_todays_call",
                                   "non_contiguous_expanded_and_side_stream"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
