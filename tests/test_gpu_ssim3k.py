"""GPU: SSIM of float32 volumes under a caller-chosen window, its gradient and the gradient of its map (rmgr_ssim_hip_*_ssim3f_win*;
ssim3k_kernels.hip for 3, 5, 7 and 9 taps, ssim3f_kernels.hip / ssim3w_kernels.hip with the window's taps for 11) against the float64
model of tests/ssim3k_model.py, and the bit patterns the header promises.  Sizes are W x H x D; arrays are (D, H, W).

Bounds.  Measured, not estimated: ssim3k_model.EMU holds, per window, what an fp32 emulation of the kernels' arithmetic leaves against
the float64 model on the golden volumes (tests/test_ssim3k_cpu.py pins the figures from both sides); everything here asserts twice those
figures -- per voxel, global, the gradient error over the volume's largest float64 gradient magnitude for both upstream forms, and
max|grad| * W * H * D * R on identical volumes.  Every test runs under the seven windows of ssimk_model.WINDOWS: every radius kernel,
and the 11-tap route with foreign taps.
"""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ssim3k_model as K3
import ssim3k_plan as PK
import ssim_amd
from conftest import ROOT
from test_gpu_ssim3f import LAYOUTS, Vol, random_pair, same

pytestmark = pytest.mark.gpu

WINDOW_IDS = [K3.name_of(w) for w in K3.WINDOWS]
WANTS = {1: (True, False), 2: (False, True), 3: (True, True)}
ENGINE = (11, 1.5, "gaussian")


def mk(window):
    """The ssim_amd.Window of a model window (size, sigma, kind); None stays None: the entries without _win."""
    if window is None:
        return None
    size, sigma, kind = window
    return ssim_amd.make_window(size, sigma if kind == "gaussian" else 1.5, kind)


def random_k(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def run(ctx, pairs, r, window, g_out=None, ks=None, scalar_k=False, want=(True, True), forward=True, maps=True, lin="dense", lk="dense",
        lout="dense", inputs=None):
    """Forward (sums, maps) and -- g_out (floats: the scalar form) or ks (volumes, or floats under strides 0 with scalar_k: the map form)
    given -- backward of `pairs` under `window` in ONE enqueue each, device-resident.  Returns (sums as float64 or None, [map], [(dA or
    None, dB or None)]).  inputs: (Vol of A, Vol of B) per pair, uploaded by the caller, instead of pairs."""
    win = mk(window)
    own = inputs is None
    if own:
        inputs = [(Vol(ctx, a.shape, lin, a), Vol(ctx, b.shape, lin, b)) for a, b in pairs]
    n = len(inputs)
    d, h, w = shape = inputs[0][0].shape
    ps = (ssim_amd.Params3F * n)()
    mvols = [Vol(ctx, shape, lout) for _ in range(n)] if forward and maps else []
    for i, (va, vb) in enumerate(inputs):
        ps[i] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides, mvols[i].ptr if mvols else None, mvols[i].strides if mvols else None)
    held, sums = [], None
    if forward:
        sums = ctx.alloc(8 * n)
        held.append(sums)
        ctx.enqueue_ssim3f(ps, n, r, sums.ptr, window=win)
    gvols, arrs = [[], []], [None, None]
    backward = g_out is not None or ks is not None
    if backward:
        for k in range(2):
            if want[k]:
                arrs[k] = (ssim_amd.Grad3F * n)()
                for i in range(n):
                    gv = Vol(ctx, shape, lout)
                    gvols[k].append(gv)
                    arrs[k][i] = ssim_amd.Grad3F(gv.ptr, *gv.strides)
        if g_out is not None:
            go = ctx.upload(np.asarray(g_out, np.float32).reshape(n))
            held.append(go)
            ctx.enqueue_ssim3f_grad(ps, n, r, go.ptr, arrs[0], arrs[1], window=win)
        else:
            ms = (ssim_amd.GradOut3F * n)()
            if scalar_k:
                one = ctx.upload(np.asarray(ks, np.float32).reshape(n))
                held.append(one)
                for i in range(n):
                    ms[i] = ssim_amd.GradOut3F(one.ptr + 4 * i, 0, 0, 0)
            else:
                kvols = [Vol(ctx, shape, lk, k) for k in ks]
                held.extend(kvols)
                for i in range(n):
                    ms[i] = ssim_amd.GradOut3F(kvols[i].ptr, *kvols[i].strides)
            ctx.enqueue_ssim3f_map_grad(ps, n, r, ms, arrs[0], arrs[1], window=win)
    ctx.synchronize()
    s = sums.download(np.float64, (n,)) if forward else None
    out_maps = [m.result() for m in mvols]
    grads = [(gvols[0][i].result() if want[0] else None, gvols[1][i].result() if want[1] else None) for i in range(n)] if backward else []
    for v in mvols + gvols[0] + gvols[1] + held:
        v.free()
    if own:
        for va, vb in inputs:
            va.free()
            vb.free()
    return s, out_maps, grads


def same_grads(x, y):
    return all((p is None and q is None) or same(p, q) for p, q in zip(x, y))


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def check_model(ctx, a, b, r, window, what, g_out=-0.75):
    """Value, map, dA alone, dB alone and both together against the float64 model at twice the emulation's figures of the window; a
    gradient has the same bits alone and together with the other."""
    px_tol, g_tol, grad_tol, ident_tol, _ = K3.tolerances(window)
    gv, gm = K3.ssim(a, b, r, window)
    ga, gb = K3.grad(a, b, r, g_out, window)
    vox = K3.voxels(a.shape)
    s, ms, both = run(ctx, [(a, b)], r, window, g_out=[g_out])
    _, _, only_a = run(ctx, [(a, b)], r, window, g_out=[g_out], want=(True, False), forward=False)
    _, _, only_b = run(ctx, [(a, b)], r, window, g_out=[g_out], want=(False, True), forward=False)
    dv, dp = abs(s[0] / vox - gv), float(np.abs(ms[0].astype(np.float64) - gm).max())
    assert same(both[0][0], only_a[0][0]) and same(both[0][1], only_b[0][1]), what
    identical = np.array_equal(a, b)
    errs = []
    for got, want in ((both[0][0], ga), (both[0][1], gb)):
        assert np.all(np.isfinite(got)), what
        errs.append(float(np.abs(got).max()) * vox * r / abs(g_out) if identical else rel(got, want))
    print("%s: per-voxel %.3g (%.3g), global %.3g (%.3g), gradients %.3g %.3g (%.3g)%s" % (
        what, dp, px_tol, dv, g_tol, errs[0], errs[1], ident_tol if identical else grad_tol, " (identical: max|grad| W H D R)" if identical else ""))
    assert dp <= px_tol and dv <= g_tol, (what, dp, dv)
    assert max(errs) <= (ident_tol if identical else grad_tol), (what, errs)


# ---- the model -----------------------------------------------------------------------------------------------------------------------

SIZES = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2),            # the axis-of-one rule on each axis
         (5, 3, 4), (9, 9, 9),                                  # axes shorter than the larger windows, tails overlapping
         (17, 17, 9),                                           # one voxel past a tile on both axes and past an 8-slice cell
         (33, 20, 13), (129, 17, 7),
         (7, 9, 300)]                                           # many z-chunks


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_model_on_every_shape_class(gpu_ctx, window, size):
    a, b = random_pair(size, sum(size))
    check_model(gpu_ctx, a, b, 1.0, window, "%s %dx%dx%d" % ((K3.name_of(window),) + size))
    if size == (33, 20, 13):
        a255, b255 = random_pair(size, sum(size) + 1, 255.0)
        check_model(gpu_ctx, a255, b255, 255.0, window, "%s %dx%dx%d at range 255" % ((K3.name_of(window),) + size), g_out=2.5)
        check_model(gpu_ctx, a, a, 1.0, window, "%s %dx%dx%d against itself" % ((K3.name_of(window),) + size), g_out=1.0)


@pytest.mark.parametrize("name", K3.FIXTURES)
@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_model_on_the_golden_volumes(gpu_ctx, manifest, window, name):
    """The forms unit and raw: value, map and the scalar gradient, and the map gradient under the three weight volumes of ssim3w_model
    (the seeds of ssim3k_model.measure())."""
    px_tol, g_tol, grad_tol, _, mapgrad_tol = K3.tolerances(window)
    seed = K3.FIXTURES.index(name)
    for form, a, b, r in K3.fixture_forms(manifest, name):
        va, vb = Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)
        gv, gm = K3.ssim(a, b, r, window)
        der = K3.derivatives(a, b, r, window)
        s, ms, gr = run(gpu_ctx, None, r, window, g_out=[1.0], inputs=[(va, vb)])
        dv, dp = abs(s[0] / K3.voxels(a.shape) - gv), float(np.abs(ms[0].astype(np.float64) - gm).max())
        errs = [rel(g, w) for g, w in zip(gr[0], K3.apply(der, 1.0 / K3.voxels(a.shape), window))]
        print("%s %s %s: per-voxel %.3g, global %.3g, gradients %.3g %.3g" % (K3.name_of(window), name, form, dp, dv, errs[0], errs[1]))
        assert dp <= px_tol and dv <= g_tol and max(errs) <= grad_tol, (name, form, dp, dv, errs)
        for wname, k in K3.weight_volumes(a.shape, seed):
            got = run(gpu_ctx, None, r, window, ks=[k], forward=False, inputs=[(va, vb)])[2][0]
            errs = [rel(g, w) for g, w in zip(got, K3.apply(der, k, window))]
            print("%s %s %s %s: map gradients %.3g %.3g of max|grad|" % (K3.name_of(window), name, form, wname, errs[0], errs[1]))
            assert all(np.all(np.isfinite(g)) for g in got) and max(errs) <= mapgrad_tol, (name, form, wname, errs)
        va.free()
        vb.free()


# ---- identities ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(17, 17, 9), (33, 20, 13)], ids=lambda s: "%dx%dx%d" % s)
def test_null_and_the_engine_window_give_the_bits_of_the_fixed_window_entries(gpu_ctx, size):
    """A NULL window (the _win entry called through ctypes with None) and {11, GAUSSIAN, 1.5f} against the entries without _win: the
    forward, the map, the gradient and the map gradient."""
    ctx = gpu_ctx
    a, b = random_pair(size, 300 + sum(size))
    k = random_k(a.shape, 301)
    fixed = run(ctx, [(a, b)], 1.0, None, g_out=[-0.75])
    fixed_map = run(ctx, [(a, b)], 1.0, None, ks=[k], forward=False)[2]
    assert np.abs(fixed[2][0][0]).max() > 0 and np.abs(fixed_map[0][1]).max() > 0
    got = run(ctx, [(a, b)], 1.0, ENGINE, g_out=[-0.75])
    assert same(got[0], fixed[0]) and same(got[1][0], fixed[1][0]) and same_grads(got[2][0], fixed[2][0])
    assert same_grads(run(ctx, [(a, b)], 1.0, ENGINE, ks=[k], forward=False)[2][0], fixed_map[0])
    # the _win entries with a NULL window
    d, h, w = a.shape
    va, vb, vk = Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b), Vol(ctx, a.shape, "dense", k)
    vm, ga, gb, ma, mb = (Vol(ctx, a.shape, "dense") for _ in range(5))
    ps, pa, pb, qa, qb, ms = (ssim_amd.Params3F * 1)(), (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)(), (ssim_amd.GradOut3F * 1)()
    ps[0] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides, vm.ptr, vm.strides)
    pa[0], pb[0], qa[0], qb[0] = (ssim_amd.Grad3F(v.ptr, *v.strides) for v in (ga, gb, ma, mb))
    ms[0] = ssim_amd.GradOut3F(vk.ptr, *vk.strides)
    sums, go = ctx.alloc(8), ctx.upload(np.float32([-0.75]))
    lib = ctx.lib
    assert lib.rmgr_ssim_hip_enqueue_ssim3f_win(ctx.handle, 1, ps, 1.0, None, sums.ptr) == 0
    assert lib.rmgr_ssim_hip_enqueue_ssim3f_win_grad(ctx.handle, 1, ps, 1.0, None, go.ptr, pa, pb) == 0
    assert lib.rmgr_ssim_hip_enqueue_ssim3f_win_map_grad(ctx.handle, 1, ps, 1.0, None, ms, qa, qb) == 0
    ctx.synchronize()
    out = (ctypes.c_float * 1)()
    assert lib.rmgr_ssim_hip_compute_ssim3f_win_device(ctx.handle, 1, ps, 1.0, None, out) == 0
    assert same(sums.download(np.float64, (1,)), fixed[0]) and same(vm.result(), fixed[1][0])
    assert same(np.float32([out[0]]), np.float32([np.float32(fixed[0][0] / K3.voxels(a.shape))]))
    assert same_grads((ga.result(), gb.result()), fixed[2][0]) and same_grads((ma.result(), mb.result()), fixed_map[0])
    for v in (va, vb, vk, vm, ga, gb, ma, mb, sums, go):
        v.free()


@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_constant_gmap_has_the_bits_of_the_scalar_gradient(gpu_ctx, window):
    """A volume of the constant float(gOut / voxels), and the one float under step, stride and sliceStride 0, against the scalar form
    for gOut under the same window: which = 1, 2, 3."""
    for size in ((17, 17, 9), (2, 1, 3)):
        a, b = random_pair(size, 100 + sum(size))
        for g_out in (-0.75, 2.5):
            kc = K3.constant_volume(g_out, a.shape)
            for which, want in WANTS.items():
                ref = run(gpu_ctx, [(a, b)], 1.0, window, g_out=[g_out], want=want, forward=False)[2]
                assert any(g is not None and np.abs(g).max() > 0 for g in ref[0])
                got = run(gpu_ctx, [(a, b)], 1.0, window, ks=[kc], want=want, forward=False)[2]
                assert same_grads(got[0], ref[0]), (size, g_out, which, "constant volume")
                got = run(gpu_ctx, [(a, b)], 1.0, window, ks=[kc.flat[0]], scalar_k=True, want=want, forward=False)[2]
                assert same_grads(got[0], ref[0]), (size, g_out, which, "one float, strides 0")


# ---- determinism -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_alone_or_anywhere_in_a_batch_and_on_a_second_call(gpu_ctx, window):
    size = (33, 20, 13)
    pairs = [random_pair(size, 40 + i) for i in range(3)]
    ks = [random_k(pairs[0][0].shape, 50 + i) for i in range(3)]
    g = [-0.75, 1.5, 0.25]
    alone = [run(gpu_ctx, [pairs[i]], 1.0, window, g_out=[g[i]]) for i in range(3)]
    alone_map = [run(gpu_ctx, [pairs[i]], 1.0, window, ks=[ks[i]], forward=False)[2][0] for i in range(3)]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        for call in range(2):                                  # a second call: the same bits
            s, ms, gr = run(gpu_ctx, [pairs[i] for i in order], 1.0, window, g_out=[g[i] for i in order])
            gm = run(gpu_ctx, [pairs[i] for i in order], 1.0, window, ks=[ks[i] for i in order], forward=False)[2]
            for pos, i in enumerate(order):
                assert same(s[pos:pos + 1], alone[i][0]) and same(ms[pos], alone[i][1][0]), (order, pos, call)
                assert same_grads(gr[pos], alone[i][2][0]) and same_grads(gm[pos], alone_map[i]), (order, pos, call)


@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "dense"])
@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_views_give_the_bits_of_the_dense_volume(gpu_ctx, window, layout):
    """Negative step, stride and sliceStride, interleaved samples (step 2) and a (D, H, W) view of data stored (H, W, D): inputs, map,
    gradients and gMap under the layout against the dense call; the sentinel gaps of the strided outputs untouched, every output voxel
    written (Vol.result)."""
    a, b = random_pair((33, 20, 13), 77)
    k = random_k(a.shape, 78)
    dense = run(gpu_ctx, [(a, b)], 1.0, window, g_out=[-0.75])
    dense_map = run(gpu_ctx, [(a, b)], 1.0, window, ks=[k], forward=False)[2][0]
    for lin, lout in ((layout, "dense"), ("dense", layout), (layout, layout)):
        s, ms, gr = run(gpu_ctx, [(a, b)], 1.0, window, g_out=[-0.75], lin=lin, lout=lout)
        assert same(s, dense[0]) and same(ms[0], dense[1][0]) and same_grads(gr[0], dense[2][0]), (lin, lout)
    for lin, lk, lout in (("dense", layout, "dense"), (layout, layout, layout)):
        got = run(gpu_ctx, [(a, b)], 1.0, window, ks=[k], forward=False, lin=lin, lk=lk, lout=lout)[2][0]
        assert same_grads(got, dense_map), (lin, lk, lout)


@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_host_entry_against_the_device_entry(gpu_ctx, window):
    a, b = random_pair((33, 20, 13), 78)
    s, ms, _ = run(gpu_ctx, [(a, b)], 1.0, window)
    want = np.float32(s[0] / K3.voxels(a.shape))
    assert abs(float(want) - K3.ssim(a, b, 1.0, window)[0]) <= K3.tolerances(window)[1]
    for ctx in (None, gpu_ctx):
        v, m = ssim_amd.compute_ssim3f(a, b, 1.0, want_map=True, ctx=ctx, window=mk(window))
        assert same(np.float32([v]), np.float32([want])) and same(m, ms[0])
    vs = ssim_amd.compute_ssim3f_batch([(a, b), (a, a)], 1.0, window=mk(window))
    assert same(vs[:1], np.float32([want])) and abs(float(vs[1]) - 1.0) < 1e-6
    va, vb = Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)
    ps = (ssim_amd.Params3F * 1)()
    ps[0] = ssim_amd.make_params3f(33, 20, 13, va.ptr, va.strides, vb.ptr, vb.strides)
    assert same(gpu_ctx.ssim3f_device(ps, 1, 1.0, window=mk(window)), np.float32([want]))
    va.free()
    vb.free()


# ---- chunk depth -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [(3, 0.0, "uniform"), (9, 1.5, "gaussian")], ids=["3 box", "9 Gaussian 1.5"])
def test_same_bits_at_every_chunk_depth(gpu_ctx, window):
    """17 x 17 x 131 alone and inside launches whose volume counts make the planner (tests/ssim3k_plan.py, held to the C++ by
    tests/test_ssim3k_cpu.py) choose at least three different chunk depths on this device -- asserted before anything is launched.
    Every sum, map and gradient of both forms has the lone launch's bits.  The largest launch (at most 64 volumes) holds about 30 MiB of
    outputs and 40 MiB of coefficient scratch."""
    ctx = gpu_ctx
    w, h, d = size = (17, 17, 131)
    R = K3.radius(window)
    said = re.search(r"(\d+) CUs", ctx.describe())
    assert said, ctx.describe()
    cus = int(said.group(1))
    counts = PK.depth_counts(R, size, cus, cap=64)
    print("chunk depths on %d CUs: %r" % (cus, [(n, g.chunk_slices) for n, g in counts]))
    assert len(counts) >= 3 and counts[0][0] == 1, counts
    pairs = [random_pair(size, 60 + i) for i in range(3)]
    ks = [random_k((d, h, w), 70 + i) for i in range(3)]
    g = [-0.75, 1.5, 0.25]
    inputs = [(Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b)) for a, b in pairs]
    alone = [run(ctx, None, 1.0, window, g_out=[g[i]], inputs=[inputs[i]]) for i in range(3)]
    alone_map = [run(ctx, None, 1.0, window, ks=[ks[i]], forward=False, inputs=[inputs[i]])[2][0] for i in range(3)]
    px_tol, g_tol, grad_tol, _, mapgrad_tol = K3.tolerances(window)
    for i in range(3):                                          # the lone launches are held to the model
        gv, gm = K3.ssim(pairs[i][0], pairs[i][1], 1.0, window)
        assert abs(alone[i][0][0] / K3.voxels(gm.shape) - gv) <= g_tol and np.abs(alone[i][1][0] - gm).max() <= px_tol
        der = K3.derivatives(pairs[i][0], pairs[i][1], 1.0, window)
        assert max(rel(x, y) for x, y in zip(alone[i][2][0], K3.apply(der, g[i] / K3.voxels(gm.shape), window))) <= grad_tol
        assert max(rel(x, y) for x, y in zip(alone_map[i], K3.apply(der, ks[i], window))) <= mapgrad_tol
    for n, geo in counts[1:]:
        pick = [(i + n) % 3 for i in range(n)]
        s, ms, gr = run(ctx, None, 1.0, window, g_out=[g[i] for i in pick], inputs=[inputs[i] for i in pick])
        gm = run(ctx, None, 1.0, window, ks=[ks[i] for i in pick], forward=False, inputs=[inputs[i] for i in pick])[2]
        for pos, i in enumerate(pick):
            assert same(s[pos:pos + 1], alone[i][0]) and same(ms[pos], alone[i][1][0]), (n, geo, pos)
            assert same_grads(gr[pos], alone[i][2][0]) and same_grads(gm[pos], alone_map[i]), (n, geo, pos)
    for v in [x for p in inputs for x in p]:
        v.free()


# ---- reach -----------------------------------------------------------------------------------------------------------------------------

def box(shape, where, radius):
    m = np.zeros(shape, bool)
    m[tuple(slice(max(p - radius, 0), p + radius + 1) for p in where)] = True
    return m


@pytest.mark.parametrize("where", [(9, 12, 13), (20, 0, 24)], ids=lambda p: "z%d y%d x%d" % p)
@pytest.mark.parametrize("window", K3.WINDOWS, ids=WINDOW_IDS)
def test_the_reach_of_a_nan(gpu_ctx, window, where):
    """25 x 23 x 21, one NaN at an interior voxel and at a corner.  A NaN sample: exactly the (2R + 1)^3 map voxels and the (4R + 1)^3
    gradient voxels around it, clipped to the volume.  A NaN in gMap: exactly (2R + 1)^3 gradient voxels.  Everything else is finite."""
    R = K3.radius(window)
    a, b = random_pair((25, 23, 21), 5)
    k = random_k(a.shape, 6)
    bad = a.copy()
    bad[where] = np.nan
    _, ms, gr = run(gpu_ctx, [(bad, b)], 1.0, window, g_out=[1.0])
    assert np.array_equal(np.isnan(ms[0]), box(a.shape, where, R)) and np.all(np.isfinite(ms[0][~box(a.shape, where, R)]))
    for g in gr[0]:
        assert np.array_equal(np.isnan(g), box(a.shape, where, 2 * R)) and np.all(np.isfinite(g[~box(a.shape, where, 2 * R)]))
    got = run(gpu_ctx, [(bad, b)], 1.0, window, ks=[k], forward=False)[2][0]
    for g in got:
        assert np.array_equal(np.isnan(g), box(a.shape, where, 2 * R)) and np.all(np.isfinite(g[~box(a.shape, where, 2 * R)]))
    kbad = k.copy()
    kbad[where] = np.nan
    got = run(gpu_ctx, [(a, b)], 1.0, window, ks=[kbad], forward=False)[2][0]
    want = K3.grad_map(a, b, 1.0, np.where(np.isnan(kbad), 0.0, kbad), window)
    inside = box(a.shape, where, R)
    for g, t in zip(got, want):
        assert np.array_equal(np.isnan(g), inside) and np.all(np.isfinite(g[~inside]))
        assert np.abs(g - t)[~inside].max() <= K3.tolerances(window)[4] * np.abs(t).max()


# ---- one context ----------------------------------------------------------------------------------------------------------------------

def test_windowed_and_fixed_window_calls_share_one_context_in_stream_order(gpu_ctx):
    """On one context, 24 enqueues -- forward, gradient and map gradient, windowed (every radius) and fixed-window, of two sizes --
    alternate without a host wait, with trim() after the twelfth: more than the 8 descriptor slots, every backward rewriting the shared
    coefficient scratch.  Every output has the bits of the same call issued alone, with a host wait, on another context."""
    ctx = gpu_ctx
    shapes = [(33, 20, 13), (20, 18, 40)]
    data = []
    for i, size in enumerate(shapes):
        a, b = random_pair(size, 200 + i)
        k = random_k(a.shape, 210 + i)
        data.append((Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b), Vol(ctx, a.shape, "dense", k), ctx.upload(np.float32([-0.75 + i]))))
    windows = [None, (3, 0.0, "uniform"), (7, 1.5, "gaussian"), (11, 2.0, "gaussian"), (5, 0.8, "gaussian"), (9, 1.5, "gaussian")]
    kinds = [(shape_i, what, win) for win in windows for shape_i, what in ((0, "forward"), (1, "grad"), (0, "map_grad"), (1, "forward"))]
    assert len(kinds) == 24

    def issue(c, calls, wait, trim_after=None):
        outs, keep = [], []
        for shape_i, what, _ in calls:                          # the outputs first: an upload waits for its context's stream
            shape = data[shape_i][0].shape
            outs.append((ctx.alloc(8), Vol(ctx, shape, "dense")) if what == "forward" else (Vol(ctx, shape, "dense"), Vol(ctx, shape, "dense")))
        ctx.synchronize()
        for pos, ((shape_i, what, win), out) in enumerate(zip(calls, outs)):
            va, vb, vk, go = data[shape_i]
            d, h, w = va.shape
            ps = (ssim_amd.Params3F * 1)()
            if what == "forward":
                ps[0] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides, out[1].ptr, out[1].strides)
                c.enqueue_ssim3f(ps, 1, 1.0, out[0].ptr, window=mk(win))
            else:
                ps[0] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides)
                pa, pb = (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)()
                pa[0], pb[0] = ssim_amd.Grad3F(out[0].ptr, *out[0].strides), ssim_amd.Grad3F(out[1].ptr, *out[1].strides)
                keep.extend((pa, pb))
                if what == "grad":
                    c.enqueue_ssim3f_grad(ps, 1, 1.0, go.ptr, pa, pb, window=mk(win))
                else:
                    ms = (ssim_amd.GradOut3F * 1)()
                    ms[0] = ssim_amd.GradOut3F(vk.ptr, *vk.strides)
                    keep.append(ms)
                    c.enqueue_ssim3f_map_grad(ps, 1, 1.0, ms, pa, pb, window=mk(win))
            keep.append(ps)
            if wait:
                c.synchronize()
            if trim_after == pos:
                c.trim()
        c.synchronize()
        got = []
        for (shape_i, what, _), out in zip(calls, outs):
            got.append((out[0].download(np.float64, (1,)), out[1].result()) if what == "forward" else (out[0].result(), out[1].result()))
            out[0].free()
            out[1].free()
        return got
    ctx.synchronize()                                          # the uploads above, before another context's stream reads them
    with ssim_amd.Context(0) as other:
        alone = issue(other, kinds, True)
    mixed = issue(ctx, kinds, False, trim_after=11)
    for i, call in enumerate(kinds):
        assert same(mixed[i][0], alone[i][0]) and same(mixed[i][1], alone[i][1]), (i, call)
    # the windows differ from one another: nothing above compared a call with itself by accident
    assert not same(alone[0][1], alone[4][1]) and not same(alone[4][1], alone[8][1])
    for item in data:
        for v in item:
            v.free()


# ---- PyTorch -----------------------------------------------------------------------------------------------------------------------------
# torch brings its own HIP runtime; the checks run in ONE child process (tests/tools/ssim3k_torch_checks.py) that imports torch before the
# library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "ssim3k_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "ssim3k_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["value_map_and_loss_against_the_conv3d_composite", "non_contiguous_expanded_sum_and_y_only",
                                   "default_keywords_are_the_call_without_keywords", "bfloat16_with_the_default_window_still_works"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
