"""GPU: multi-scale SSIM of float32 samples under a caller-chosen window and its gradient (rmgr_ssim_hip_enqueue_msssimf_win,
rmgr_ssim_hip_compute_msssimf_win_device / _host, rmgr_ssim_hip_enqueue_msssimf_win_grad, ssim_amd.torch_ops.ms_ssim(win_size=...)) against
the float64 definition (tests/msssimk_model.py), and their determinism.

Bounds.  Measured, not estimated, and fixed before the first GPU run: per window an fp32 emulation of the kernels' arithmetic
(msssimk_model.Emulation) is measured against the float64 model on ssimk_model.FIXTURES in two forms at Wang's 5 scales and at uniform
weights for 1, 3 and 8 scales (msssimk_model.EMU; tests/test_msssimk_cpu.py pins the figures); the bound is ssimk_model.TOL_FACTOR (2.0)
times the figure.  The odd sizes have figures of their own, measured the same way on their own inputs (msssimk_model.ODD_EMU).  What the
MI355X itself left is written beside them in msssimk_model.GPU.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msssimk_inputs as IN
import msssimk_model as MK
import ssimk_model as SK
import ssim_amd
from conftest import ROOT, load_pair
from msssimk_inputs import DevicePairs, bits, mk, same

pytestmark = pytest.mark.gpu

BY_WINDOW = pytest.mark.parametrize("window", SK.WINDOWS, ids=SK.name_of)
G_OUT = -0.75


def host(a, b, r, window, scales=5, weights=None):
    return ssim_amd.compute_msssimf(a, b, r, scales, weights, per_scale=True, window=mk(window))


# ---- 1. against the float64 model ----

@BY_WINDOW
def test_fixtures_in_two_forms_at_wang_and_uniform_scales(gpu_ctx, manifest, window):
    """The seven windows (the 11-tap box and 11 Gaussian 2 run the kernels of msssimf_kernels.hip with other taps) on the five fixtures in
    two forms: value, every per-scale mean, both gradients, and the pair of identical images."""
    tv, tm, tg, ti = MK.tolerances(window)
    win = mk(window)
    wv = wm = wg = wi = 0.0
    for name in SK.FIXTURES:
        for form, fa, fb, r in SK.fixture_forms(manifest, name):
            mod = MK.model(fa, fb, r, window)
            dp, same_dp = DevicePairs(gpu_ctx, [(fa, fb)]), DevicePairs(gpu_ctx, [(fa, fa)])
            for scales, w in MK.CONFIGS:
                v, means = host(fa, fb, r, window, scales, w)
                got = dp.grads(r, win, [G_OUT], scales, w)[0]
                assert all(np.all(np.isfinite(g)) for g in got)
                fv, fm, fg = MK.figures(v, means, got, mod, scales, w, G_OUT)
                fi = MK.ident_figure(same_dp.grads(r, win, [G_OUT], scales, w)[0], fa.shape, r, G_OUT)
                print("%s %s/%s, %d scales: value %.3g mean %.3g grad %.3g identical %.3g" % (SK.name_of(window), name, form, scales, fv, fm, fg, fi))
                wv, wm, wg, wi = max(wv, fv), max(wm, fm), max(wg, fg), max(wi, fi)
            dp.free()
            same_dp.free()
    print("GPU %r: (%.3e, %.3e, %.3e, %.3e)" % (window, wv, wm, wg, wi))
    assert wv <= tv and wm <= tm and wg <= tg and wi <= ti, (window, (wv, wm, wg, wi), (tv, tm, tg, ti))


@pytest.mark.parametrize("window", [IN.BOX3, IN.G9], ids=SK.name_of)
def test_odd_sizes_whose_planes_are_smaller_than_the_window(gpu_ctx, window):
    """(1, 1), (3, 5), (17, 33) and (7, 300) at 1 .. 8 scales; (40, 300) at 4 scales (two strip columns at scale 1); (9, 603) at 3 scales
    (multi-cell strips): coarse planes clamp under the window, down to 1 x 1."""
    tv, tm, tg = (SK.TOL_FACTOR * x for x in MK.ODD_EMU[window])
    win = mk(window)
    wv = wm = wg = 0.0
    for h, w, configs, a, b, r in IN.odd_cases():
        mod = MK.model(a, b, r, window)
        dp = DevicePairs(gpu_ctx, [(a, b)])
        for scales in configs:
            wts = (1.0 / scales,) * scales
            v, means = host(a, b, r, window, scales, wts)
            got = dp.grads(r, win, [IN.ODD_G_OUT], scales, wts)[0]
            assert all(g.shape == (h, w) and np.all(np.isfinite(g)) for g in got)
            fv, fm, fg = MK.figures(v, means, got, mod, scales, wts, IN.ODD_G_OUT)
            print("%s %dx%d/%g, %d scales: value %.3g mean %.3g grad %.3g" % (SK.name_of(window), w, h, r, scales, fv, fm, fg))
            wv, wm, wg = max(wv, fv), max(wm, fm), max(wg, fg)
        dp.free()
    print("GPU odd %r: (%.3e, %.3e, %.3e)" % (window, wv, wm, wg))
    assert wv <= tv and wm <= tm and wg <= tg, (window, (wv, wm, wg), (tv, tm, tg))


# ---- 2. the default window is msssimf ----

def test_null_and_the_engines_window_give_the_bits_of_msssimf(gpu_ctx, manifest):
    a, b = load_pair(manifest["bbb257x65_q50_ch1"])
    fa, fb = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
    ctx, lib = gpu_ctx, gpu_ctx.lib
    dp = DevicePairs(ctx, [(fa, fb), (fb, fa)])
    for scales, w in ((5, None), (3, (0.2, 0.3, 0.5)), (1, (1.0,))):
        v0, m0 = dp.forward(1.0, None, scales, w)
        g0 = dp.grads(1.0, None, [G_OUT, 0.5], scales, w)
        h0 = ssim_amd.compute_msssimf_batch([(fa, fb), (fb, fa)], 1.0, scales, w, per_scale=True)
        engine = mk(SK.DEFAULT)
        v1, m1 = dp.forward(1.0, engine, scales, w)
        g1 = dp.grads(1.0, engine, [G_OUT, 0.5], scales, w)
        h1 = ssim_amd.compute_msssimf_batch([(fa, fb), (fb, fa)], 1.0, scales, w, per_scale=True, window=engine)
        d1 = dp.device(1.0, engine, scales, w)
        assert same(v1, v0) and same(m1, m0) and same(h1[0], h0[0]) and same(h1[1], h0[1]) and same(d1[0], h0[0]) and same(d1[1], h0[1])
        for i in range(2):
            assert same(g1[i][0], g0[i][0]) and same(g1[i][1], g0[i][1])
        # a NULL window through the _win entries themselves (the binding's window=None calls the entries without _win)
        wts = None if w is None else (ctypes.c_double * scales)(*w)
        vals, means, go = ctx.alloc(16), ctx.alloc(32 * scales), ctx.upload(np.float32([G_OUT, 0.5]))
        arrs, bufs, fill = dp.grad_planes()
        assert lib.rmgr_ssim_hip_enqueue_msssimf_win(ctx.handle, 2, dp.params, 1.0, None, scales, wts, vals.ptr, means.ptr) == 0
        assert lib.rmgr_ssim_hip_enqueue_msssimf_win_grad(ctx.handle, 2, dp.params, 1.0, None, scales, wts, means.ptr, go.ptr, arrs[0], arrs[1]) == 0
        ctx.synchronize()
        assert same(vals.download(np.float64, (2,)), v0) and same(means.download(np.float64, (2, scales, 2)), m0)
        g2 = dp.collect(arrs, bufs, fill)
        for i in range(2):
            assert same(g2[i][0], g0[i][0]) and same(g2[i][1], g0[i][1])
        out = (ctypes.c_float * 2)()
        hm = (ctypes.c_double * (4 * scales))()
        assert lib.rmgr_ssim_hip_compute_msssimf_win_device(ctx.handle, 2, dp.params, 1.0, None, scales, wts, out, hm) == 0
        assert same(np.array(out[:], np.float32), h0[0]) and same(np.array(hm[:], np.float64).reshape(2, scales, 2), h0[1])
        for x in (vals, means, go):
            x.free()
    dp.free()


# ---- 3. determinism ----

def pool_pairs(manifest):
    out = []
    for n in ("bbb257x65_q00_ch1", "bbb257x65_q50_ch1"):
        a, b = load_pair(manifest[n])
        fa, fb = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
        out += [(fa, fb), (fb, fa), (fa[::-1].copy(), fb[::-1].copy())]
    return out


@pytest.mark.parametrize("window", [(7, 0.0, "uniform"), (5, 0.8, "gaussian")], ids=SK.name_of)
def test_same_bits_alone_in_a_batch_through_every_entry_and_with_one_gradient_or_both(gpu_ctx, manifest, window):
    win = mk(window)
    pool = pool_pairs(manifest)
    pair = pool[1]
    hv, hm = host(pair[0], pair[1], 1.0, window)
    alone = DevicePairs(gpu_ctx, [pair])
    v1, m1 = alone.forward(1.0, win)
    g1 = alone.grads(1.0, win, [0.5])[0]
    v1b, m1b = alone.forward(1.0, win)                                                   # repeated calls
    assert same(v1b, v1) and same(m1b, m1)
    only_a, only_b = alone.grads(1.0, win, [0.5], want_b=False)[0], alone.grads(1.0, win, [0.5], want_a=False)[0]
    assert only_a[1] is None and only_b[0] is None and same(only_a[0], g1[0]) and same(only_b[1], g1[1])
    dv, dm = alone.device(1.0, win)                                                      # _device, _host, enqueue
    assert np.float32(v1[0]) == hv == dv[0] and same(m1[0], hm) and same(dm[0], hm)
    alone.free()
    n, at = 7, 3
    pairs = [pool[i % len(pool)] for i in range(n)]
    pairs[at] = pair
    g_out = [0.25 * (i - at) + 0.5 for i in range(n)]                                    # differs per pair, 0 and negatives included
    dp = DevicePairs(gpu_ctx, pairs)
    v, m = dp.forward(1.0, win)
    g = dp.grads(1.0, win, g_out)
    vals, means = dp.device(1.0, win)
    dp.free()
    assert bits(v)[at] == bits(v1)[0] and same(m[at], m1[0]) and vals[at] == hv
    assert same(g[at][0], g1[0]) and same(g[at][1], g1[1])
    hvals, hmeans = ssim_amd.compute_msssimf_batch(pairs, 1.0, per_scale=True, window=win)
    assert same(hvals, vals) and same(hmeans, means) and same(means, m)
    assert not bits(g[1][0]).any() and not bits(g[1][1]).any()                           # gOut == 0: +0 everywhere


def test_device_batch_that_is_split_into_sub_batches(gpu_ctx):
    """200 pairs of 1920 x 1080 need 5.6 MB each of pyramid and partials: the forward runs in two sub-batches; 140 of them with dLoss/dA
    alone need 8.3 MB each: so does the backward.  Every pair reads the same two device images and writes a gradient plane of its own."""
    from ssim_amd import synth
    win = mk((7, 0.0, "uniform"))
    a, b = synth.pair_numpy(1920, 1080, 5)
    fa, fb = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
    h, w, nf, n = 1080, 1920, 200, 140
    one = DevicePairs(gpu_ctx, [(fa, fb)])
    want = one.grads(1.0, win, [0.7], want_b=False)[0][0]
    v1, m1 = one.forward(1.0, win)
    params = (ssim_amd.ParamsF * nf)()
    for i in range(nf):
        params[i] = one.params[0]
    vals, means, go = gpu_ctx.alloc(8 * nf), gpu_ctx.alloc(80 * nf), gpu_ctx.upload(np.full(n, 0.7, np.float32))
    out = gpu_ctx.alloc(4 * h * w * n)
    ga = (ssim_amd.GradF * n)()
    for i in range(n):
        ga[i] = ssim_amd.GradF(out.ptr + 4 * h * w * i, 1, w)
    gpu_ctx.enqueue_msssimf(params, nf, 1.0, vals.ptr, means.ptr, window=win)
    gpu_ctx.enqueue_msssimf_grad(params, n, 1.0, means.ptr, go.ptr, ga, None, window=win)
    gpu_ctx.synchronize()
    v, m = vals.download(np.float64, (nf,)), means.download(np.float64, (nf, 5, 2))
    assert np.all(bits(v) == bits(v1)[0]) and all(same(m[i], m1[0]) for i in range(nf))
    lib = gpu_ctx.lib
    for i in (0, 127, 128, 129, 139):
        plane = np.empty((h, w), np.float32)
        assert lib.rmgr_ssim_hip_memcpy_d2h(gpu_ctx.handle, plane.ctypes.data, out.ptr + 4 * h * w * i, plane.nbytes) == 0
        assert same(plane, want), i
    for x in (vals, means, go, out):
        x.free()
    one.free()


@pytest.mark.parametrize("window", [IN.BOX3, IN.G9], ids=SK.name_of)
def test_views_with_negative_and_interleaved_steps(gpu_ctx, manifest, window):
    win = mk(window)
    a, b = load_pair(manifest["bbb257x65_q50_ch1"])
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    v, m = host(fa, fb, 255.0, window)
    ra, rb = np.ascontiguousarray(fa[::-1, ::-1]), np.ascontiguousarray(fb[::-1, ::-1])
    v2, m2 = host(ra[::-1, ::-1], rb[::-1, ::-1], 255.0, window)                         # negative steps on the host
    assert v2 == v and same(m2, m)
    rgb_a, rgb_b = np.zeros(fa.shape + (3,), np.float32), np.zeros(fa.shape + (3,), np.float32)
    rgb_a[:, :, 1], rgb_b[:, :, 1] = fa, fb
    v3, m3 = host(rgb_a[:, :, 1], rgb_b[:, :, 1], 255.0, window)                         # channel-interleaved storage
    assert v3 == v and same(m3, m)
    plain = DevicePairs(gpu_ctx, [(fa, fb)])
    g = plain.grads(255.0, win, [1.0])[0]
    assert same(plain.forward(255.0, win)[1][0], m)
    plain.free()
    inter = DevicePairs(gpu_ctx, [(fa, fb)], step=3, lead=5)
    g3 = inter.grads(255.0, win, [1.0], gstep=2, lead=3)[0]
    assert same(inter.forward(255.0, win)[1][0], m)
    inter.free()
    assert same(g3[0], g[0]) and same(g3[1], g[1])
    # negative steps on the device: the flipped image addressed from its last sample, the gradient plane likewise
    h, w = fa.shape
    da, db = gpu_ctx.upload(ra), gpu_ctx.upload(rb)
    ps = (ssim_amd.ParamsF * 1)()
    last = 4 * (h * w - 1)
    ps[0] = ssim_amd.make_params_f(w, h, da.ptr + last, -1, -w, db.ptr + last, -1, -w)
    dv, dm = gpu_ctx.msssimf_device(ps, 1, 255.0, per_scale=True, window=win)
    assert dv[0] == v and same(dm[0], m)
    vals, means = gpu_ctx.alloc(8), gpu_ctx.alloc(80)
    go, out = gpu_ctx.upload(np.ones(1, np.float32)), gpu_ctx.alloc(4 * h * w)
    ga = (ssim_amd.GradF * 1)()
    ga[0] = ssim_amd.GradF(out.ptr + last, -1, -w)
    gpu_ctx.enqueue_msssimf(ps, 1, 255.0, vals.ptr, means.ptr, window=win)
    gpu_ctx.enqueue_msssimf_grad(ps, 1, 255.0, means.ptr, go.ptr, ga, None, window=win)
    gpu_ctx.synchronize()
    flipped = out.download(np.float32, (h, w))
    for x in (da, db, go, out, vals, means):
        x.free()
    assert same(flipped[::-1, ::-1], g[0])


# ---- 4. the 64-bit forms ----

@pytest.mark.parametrize("window", IN.PER_RADIUS, ids=SK.name_of)
@pytest.mark.parametrize("sign", [1, -1], ids=["forwards", "backwards"])
def test_64_bit_form_with_planes_far_apart(gpu_ctx, window, sign):
    """One 9 x 5 (H x W) pair at 2 scales with samples 2^21 floats apart -- the first step fitsf_narrow() refuses --: the bits of the
    dense call, and nothing but the gradient planes written."""
    win = mk(window)
    a, b = IN.random_pair(9, 5, np.random.default_rng(33))
    g_out, scales, wts = [45.0], 2, (0.4, 0.6)
    dense = DevicePairs(gpu_ctx, [(a, b)])
    v, m = dense.forward(1.0, win, scales, wts)
    g = dense.grads(1.0, win, g_out, scales, wts)[0]
    dense.free()
    fv, fm, da, db, untouched = IN.far_apart_call(gpu_ctx, "f", (a, b), 1 << 21, sign, 1.0, win, g_out, scales, wts, np.float32(np.nan))
    assert same(fv, v) and same(fm, m) and same(da, g[0]) and same(db, g[1]) and untouched


# ---- 5. the context's scratch between a forward and its backward ----

def test_a_default_window_forward_between_a_windowed_forward_and_its_backward(gpu_ctx):
    """The windowed forward, a default-window forward of another shape on the same context (it overwrites the pyramid and the partials),
    then the windowed backward: the backward recomputes its pyramid, so the gradient has the bits of the undisturbed sequence."""
    rng = np.random.default_rng(21)
    win = mk((7, 1.5, "gaussian"))
    a, b = IN.random_pair(70, 300, rng)
    other = IN.random_pair(129, 127, rng)
    dp, od = DevicePairs(gpu_ctx, [(a, b)]), DevicePairs(gpu_ctx, [other, other])
    want = dp.grads(1.0, win, [G_OUT])[0]
    v, m, means = dp.forward(1.0, win, keep=True)
    ov, om = od.forward(1.0, None)
    assert np.all(np.isfinite(ov))
    go = gpu_ctx.upload(np.float32([G_OUT]))
    arrs, bufs, fill = dp.grad_planes()
    dp.enqueue_grad(1.0, means.ptr, go.ptr, arrs[0], arrs[1], 5, None, win)
    gpu_ctx.synchronize()
    got = dp.collect(arrs, bufs, fill)[0]
    assert same(got[0], want[0]) and same(got[1], want[1])
    for x in (go, means):
        x.free()
    dp.free()
    od.free()


# ---- 6. NaN and the ReLU ----

@pytest.mark.parametrize("window", [IN.BOX3, (11, 0.0, "uniform")], ids=SK.name_of)
def test_nan_sample_gives_a_nan_value(window):
    a, b = IN.random_pair(64, 300, np.random.default_rng(9))
    clean = host(a, b, 1.0, window)[0]
    a[31, 70] = np.nan
    v, means = host(a, b, 1.0, window)
    assert np.isnan(v) and np.isnan(means[:, 0]).all() and np.isfinite(clean)
    both = ssim_amd.compute_msssimf_batch([(a, b), (b, b)], 1.0, window=mk(window))
    assert np.isnan(both[0]) and abs(float(both[1]) - 1.0) <= 1e-6


@pytest.mark.parametrize("window", [IN.BOX3, IN.G9], ids=SK.name_of)
def test_relu_pair_is_zero_with_an_all_zero_gradient(gpu_ctx, manifest, window):
    win = mk(window)
    a, _ = load_pair(manifest["bbb257x65_q00_ch1"])
    fa = a.astype(np.float32)
    fb = (np.float32(255.0) - fa).astype(np.float32)
    v, means = host(fa, fb, 255.0, window)
    assert bits(np.float32(v)) == 0 and np.all(means[:-1, 0] < 0) and MK.model(fa, fb, 255.0, window).msssim()[0] == 0.0, (float(v), means)
    dp = DevicePairs(gpu_ctx, [(fa, fb), (fa, fa)])
    (ga, gb), (ia, ib) = dp.grads(255.0, win, [1.0, 1.0])
    dp.free()
    assert not bits(ga).any() and not bits(gb).any()                       # +0 everywhere, bit for bit: no NaN, no -0
    assert np.all(np.isfinite(ia)) and np.all(np.isfinite(ib))             # its batch neighbour is untouched by it


# ---- torch ----
# torch brings a HIP runtime of its own, which has to be the first one a process loads: the checks run in one child process
# (tests/tools/msssimk_torch_checks.py) that imports torch before the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "msssimk_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "msssimk_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["windowed_ms_ssim_is_the_c_abi_bit_for_bit", "windowed_ms_ssim_amp_on_bfloat16_is_the_c_abi_bit_for_bit",
                                   "loss_under_autocast_hands_out_a_bfloat16_gradient", "default_keywords_give_the_bits_of_todays_call",
                                   "non_contiguous_slice_and_side_stream"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
