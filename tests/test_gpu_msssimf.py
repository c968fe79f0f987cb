"""GPU: multi-scale SSIM of float32 samples and its gradient (rmgr_ssim_hip_enqueue_msssimf, rmgr_ssim_hip_compute_msssimf_device / _host,
rmgr_ssim_hip_enqueue_msssimf_grad, ssim_amd.torch_ops.ms_ssim) against the float64 definition (tests/msssimf_model.py), and their
determinism.

Bounds.  Measured, not estimated: an fp32 emulation of the kernels' arithmetic (msssimf_model.Emulation) lands within 1.172e-6 of the
model on the value, 1.602e-6 on every per-scale mean and 2.648e-4 of the plane's largest float64 gradient magnitude on every golden pair
in three forms (/ 255 at range 1, as stored at range 255, scaled by a non-integer factor to range 1000) at Wang's 5 scales and at 1 .. 8
scales with uniform weights, and leaves max|grad| * W * H * R = 3.648e-4 on the pair of identical images, whose exact gradient is 0
(tests/test_msssimf_cpu.py pins these figures).  The asserted bounds are about twice that: VALUE_TOL = 2.5e-6, MEAN_TOL = 3.4e-6,
GRAD_TOL = 5.5e-4, IDENT_TOL = 7.5e-4.  The MI355X itself measured 1.15e-6, 1.60e-6, 2.65e-4 and 3.65e-4 on those cases.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msssimf_model as M
import ssimf_model as SF
import ssim_amd
from conftest import ROOT, image_entries, load_pair
from msssimf_model import GRAD_TOL, IDENT_TOL, MEAN_TOL, VALUE_TOL

pytestmark = pytest.mark.gpu

MS8_TOL = 3e-6              # the uint8 multi-scale path's bound (tests/test_gpu_msssim.py)
CONFIGS = [(5, None)] + [(m, (1.0 / m,) * m) for m in range(1, 9)]      # Wang's five; uniform weights at 1 .. 8 scales
SMALL = [(1, 1), (3, 5), (17, 33), (65, 257), (129, 127), (7, 300)]     # (H, W)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if np.asarray(x).dtype == np.float32 else np.uint64)


def random_pair(h, w, rng, r=1.0):
    a = rng.random((h, w), dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal((h, w)).astype(np.float32), 0, 1).astype(np.float32)
    return a * np.float32(r), b * np.float32(r)


class DevicePairs(object):
    """Pairs of one size in device memory, each image in a buffer of its own, at any step (samples interleaved `step` apart)."""

    def __init__(self, ctx, pairs, step=1):
        self.ctx, self.n, self.step = ctx, len(pairs), step
        self.h, self.w = pairs[0][0].shape
        self.bufs = []
        self.params = (ssim_amd.ParamsF * self.n)()
        for i, (a, b) in enumerate(pairs):
            d = []
            for img in (a, b):
                wide = np.zeros((self.h, self.w, step), np.float32)
                wide[:, :, step - 1] = img
                d.append(ctx.upload(wide))
            self.bufs += d
            off = 4 * (step - 1)
            self.params[i] = ssim_amd.make_params_f(self.w, self.h, d[0].ptr + off, step, self.w * step, d[1].ptr + off, step, self.w * step)

    def forward(self, r, scales=5, weights=None, keep=False):
        """(values float64 (n,), means float64 (n, scales, 2)) through rmgr_ssim_hip_enqueue_msssimf; keep: also the device buffer of the means."""
        vals, means = self.ctx.alloc(8 * self.n), self.ctx.alloc(16 * self.n * scales)
        self.ctx.enqueue_msssimf(self.params, self.n, r, vals.ptr, means.ptr, scales, weights)
        self.ctx.synchronize()
        v, m = vals.download(np.float64, (self.n,)), means.download(np.float64, (self.n, scales, 2))
        vals.free()
        if keep:
            return v, m, means
        means.free()
        return v, m

    def grads(self, r, g_out, scales=5, weights=None, want_a=True, want_b=True, gstep=1, means=None):
        """[(dLoss/dA or None, dLoss/dB or None)] per pair, forward then backward; gradient planes with samples gstep apart, the gaps
        checked untouched.  means: a float64 (n, scales, 2) array handed to the backward in place of this forward's."""
        ctx, n, h, w = self.ctx, self.n, self.h, self.w
        if means is None:
            _, _, means = self.forward(r, scales, weights, keep=True)
        else:
            means = np.ascontiguousarray(means, np.float64)
            assert means.shape == (n, scales, 2)
            means = ctx.upload(means)
        go = ctx.upload(np.asarray(g_out, np.float32))
        fill = np.full((h, w, gstep), -777.0, np.float32)
        arrs, bufs = [None, None], [[], []]
        for k, want in enumerate((want_a, want_b)):
            if not want:
                continue
            arrs[k] = (ssim_amd.GradF * n)()
            for i in range(n):
                buf = ctx.upload(fill)
                bufs[k].append(buf)
                arrs[k][i] = ssim_amd.GradF(buf.ptr, gstep, w * gstep)
        ctx.enqueue_msssimf_grad(self.params, n, r, means.ptr, go.ptr, arrs[0], arrs[1], scales, weights)
        ctx.synchronize()
        out = []
        for i in range(n):
            pair = []
            for k in range(2):
                if arrs[k] is None:
                    pair.append(None)
                    continue
                g = bufs[k][i].download(np.float32, (h, w, gstep))
                assert np.all(g[:, :, 1:] == -777.0)
                pair.append(np.ascontiguousarray(g[:, :, 0]))
            out.append(tuple(pair))
        for b in bufs[0] + bufs[1] + [go, means]:
            b.free()
        return out

    def free(self):
        for b in self.bufs:
            b.free()


def check_forward(got_v, got_m, mod, scales, weights, what):
    mv, mm = mod.msssim(scales, weights)
    dv, dm = abs(float(got_v) - mv), float(np.abs(np.asarray(got_m) - mm).max())
    print("%s, %d scales: value %.3g, per-scale means %.3g" % (what, scales, dv, dm))
    assert dv <= VALUE_TOL, (what, scales, float(got_v), mv)
    assert dm <= MEAN_TOL, (what, scales, got_m, mm)


def check_grad(got, mod, r, g_out, scales, weights, what, identical=False):
    ga, gb = mod.grad(g_out, scales, weights)
    for name, g, want in (("dA", got[0], ga), ("dB", got[1], gb)):
        if g is None:
            continue
        assert g.shape == want.shape and np.all(np.isfinite(g)), (what, name)
        if g_out == 0:
            assert np.all(g == 0), (what, name)
        elif identical:
            e = float(np.abs(g).max()) * g.size * r / abs(g_out)
            print("%s %s, %d scales: identical images, max|grad| W H R = %.3g" % (what, name, scales, e))
            assert e <= IDENT_TOL, (what, name, scales, e)
        else:
            e = float(np.abs(g - want).max() / np.abs(want).max())
            print("%s %s, %d scales: %.3g of max|grad|" % (what, name, scales, e))
            assert e <= GRAD_TOL, (what, name, scales, e)


# ---- against the float64 model ----

def test_golden_fixtures_in_three_forms_at_wang_and_uniform_scales(gpu_ctx, manifest):
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        for form, fa, fb, r in M.forms(a, b):
            mod = M.Model(fa, fb, r)
            dp = DevicePairs(gpu_ctx, [(fa, fb)])
            for scales, w in CONFIGS:
                what = "%s/%s" % (n, form)
                v, means = ssim_amd.compute_msssimf(fa, fb, r, scales, w, per_scale=True)
                check_forward(v, means, mod, scales, w, what)
                check_grad(dp.grads(r, [1.0], scales, w)[0], mod, r, 1.0, scales, w, what, identical=np.array_equal(a, b))
            dp.free()


def test_small_and_odd_sizes_down_to_one_pixel(gpu_ctx):
    """Odd sizes at every scale (257 x 65 -> 129 x 33 -> 65 x 17 -> 33 x 9 -> 17 x 5; 33 x 17; 5 x 3), a single row of cells, 1 x 1."""
    rng = np.random.default_rng(7)
    for (h, w) in SMALL:
        for r in (1.0, 255.0):
            a, b = random_pair(h, w, rng, r)
            mod = M.Model(a, b, r)
            dp = DevicePairs(gpu_ctx, [(a, b)])
            for scales, wts in ((5, None), (8, (0.125,) * 8), (3, (0.5, 0.0, 0.5))):
                what = "%dx%d/%g" % (w, h, r)
                v, means = ssim_amd.compute_msssimf(a, b, r, scales, wts, per_scale=True)
                check_forward(v, means, mod, scales, wts, what)
                check_grad(dp.grads(r, [-0.75], scales, wts)[0], mod, r, -0.75, scales, wts, what)
            dp.free()


def test_1080p_and_4096_square(gpu_ctx):
    from ssim_amd import synth
    for (w, h) in ((1920, 1080), (4096, 4096)):
        a, b = synth.pair_numpy(w, h)
        fa, fb = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
        mod = M.Model(fa, fb, 1.0)
        v, means = ssim_amd.compute_msssimf(fa, fb, 1.0, per_scale=True)
        check_forward(v, means, mod, 5, None, "synth %dx%d" % (w, h))
        if w == 1920:
            dp = DevicePairs(gpu_ctx, [(fa, fb)])
            got = dp.grads(1.0, [-1.0])[0]
            dp.free()
            check_grad(got, mod, 1.0, -1.0, 5, None, "synth 1920x1080")


# ---- ties to the existing paths ----

def test_integer_valued_floats_agree_with_the_uint8_path(manifest):
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        for scales, w in ((5, None), (3, (0.2, 0.3, 0.5))):
            vf, mf = ssim_amd.compute_msssimf(a.astype(np.float32), b.astype(np.float32), 255.0, scales, w, per_scale=True)
            v8, m8 = ssim_amd.compute_msssim(a, b, scales, w, per_scale=True)
            assert abs(float(vf) - float(v8)) <= VALUE_TOL + MS8_TOL, (n, scales, float(vf), float(v8))
            assert np.abs(mf - m8).max() <= MEAN_TOL + MS8_TOL, (n, scales, mf, m8)


def test_one_scale_of_weight_one_agrees_with_ssimf(gpu_ctx, manifest):
    for n in ("einstein_jpg", "bbb257x65_q50_ch1", "einstein_meanshift"):
        a, b = load_pair(manifest[n])
        fa, fb = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
        h, w = fa.shape
        v, means = ssim_amd.compute_msssimf(fa, fb, 1.0, 1, (1.0,), per_scale=True)
        vs, _ = ssim_amd.compute_ssimf(fa, fb, 1.0)
        assert abs(float(v) - float(vs)) <= VALUE_TOL + SF.G_TOL and abs(means[0][1] - float(vs)) <= MEAN_TOL + SF.G_TOL, (n, float(v), float(vs))
        dp = DevicePairs(gpu_ctx, [(fa, fb)])
        ga, gb = dp.grads(1.0, [1.0], 1, (1.0,))[0]
        go, oa, ob = gpu_ctx.upload(np.ones(1, np.float32)), gpu_ctx.alloc(4 * h * w), gpu_ctx.alloc(4 * h * w)
        pa, pb = (ssim_amd.GradF * 1)(), (ssim_amd.GradF * 1)()
        pa[0], pb[0] = ssim_amd.GradF(oa.ptr, 1, w), ssim_amd.GradF(ob.ptr, 1, w)
        gpu_ctx.enqueue_ssimf_grad(dp.params, 1, 1.0, go.ptr, pa, pb)
        gpu_ctx.synchronize()
        sa, sb = oa.download(np.float32, (h, w)), ob.download(np.float32, (h, w))
        for x in (go, oa, ob):
            x.free()
        dp.free()
        wa, wb = SF.grad(fa, fb, 1.0, 1.0)
        for g, s, want in ((ga, sa, wa), (gb, sb, wb)):
            assert np.abs(g.astype(np.float64) - s).max() <= (GRAD_TOL + SF.GRAD_TOL) * np.abs(want).max(), n


# ---- the ReLU and NaN ----

def test_relu_pair_is_zero_with_an_all_zero_gradient(gpu_ctx, manifest):
    a, _ = load_pair(manifest["einstein_jpg"])
    for fa, r in ((a.astype(np.float32), 255.0), (a.astype(np.float32) / np.float32(255), 1.0)):
        fb = (np.float32(r) - fa).astype(np.float32)
        v, means = ssim_amd.compute_msssimf(fa, fb, r, per_scale=True)
        assert bits(np.float32(v)) == 0 and np.all(means[:, 0] < -0.3), (float(v), means)
        dp = DevicePairs(gpu_ctx, [(fa, fb), (fa, fa)])
        (ga, gb), (ia, ib) = dp.grads(r, [1.0, 1.0])
        dp.free()
        assert not bits(ga).any() and not bits(gb).any()                   # +0 everywhere, bit for bit: no NaN, no -0
        assert np.all(np.isfinite(ia)) and np.all(np.isfinite(ib))         # its batch neighbour is untouched by it


def test_nan_sample_gives_nan():
    rng = np.random.default_rng(9)
    a, b = random_pair(64, 300, rng)
    clean = ssim_amd.compute_msssimf(a, b, 1.0)
    a[31, 70] = np.nan
    v, means = ssim_amd.compute_msssimf(a, b, 1.0, per_scale=True)
    assert np.isnan(v) and np.isnan(means[:, 0]).all() and np.isfinite(clean)
    both = ssim_amd.compute_msssimf_batch([(a, b), (b, b)], 1.0)
    assert np.isnan(both[0]) and abs(float(both[1]) - 1.0) <= 1e-6


# ---- determinism ----

def einstein_pairs(manifest):
    out = []
    for n in image_entries(manifest):
        if n.startswith("einstein_") and n != "einstein_einstein":
            a, b = load_pair(manifest[n])
            out.append((a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)))
    return out


def test_same_bits_alone_in_batches_on_every_call_and_with_one_gradient_or_both(gpu_ctx, manifest):
    pool = einstein_pairs(manifest)
    pair = pool[0]
    hv, hm = ssim_amd.compute_msssimf(pair[0], pair[1], 1.0, per_scale=True)
    alone = DevicePairs(gpu_ctx, [pair])
    v1, m1 = alone.forward(1.0)
    g1 = alone.grads(1.0, [0.5])[0]
    v1b, m1b = alone.forward(1.0)                                                         # repeated calls
    assert np.array_equal(bits(v1b), bits(v1)) and np.array_equal(bits(m1b), bits(m1))
    g1b = alone.grads(1.0, [0.5])[0]
    assert np.array_equal(bits(g1b[0]), bits(g1[0])) and np.array_equal(bits(g1b[1]), bits(g1[1]))
    only_a, only_b = alone.grads(1.0, [0.5], want_b=False)[0], alone.grads(1.0, [0.5], want_a=False)[0]
    assert only_a[1] is None and only_b[0] is None
    assert np.array_equal(bits(only_a[0]), bits(g1[0])) and np.array_equal(bits(only_b[1]), bits(g1[1]))
    dv, dm = gpu_ctx.msssimf_device(alone.params, 1, 1.0, per_scale=True)                 # every entry point
    assert np.float32(v1[0]) == hv == dv[0] and np.array_equal(bits(m1[0]), bits(hm)) and np.array_equal(bits(dm[0]), bits(hm))
    alone.free()
    for n in (2, 7, 33):
        at = n // 2
        pairs = [pool[(i + 1) % len(pool)] for i in range(n)]
        pairs[at] = pair
        g_out = [0.25 * (i - at) + 0.5 for i in range(n)]                                 # differs per pair, 0 and negatives included
        dp = DevicePairs(gpu_ctx, pairs)
        v, m = dp.forward(1.0)
        g = dp.grads(1.0, g_out)
        vals, means = gpu_ctx.msssimf_device(dp.params, n, 1.0, per_scale=True)
        dp.free()
        assert bits(v)[at] == bits(v1)[0] and np.array_equal(bits(m[at]), bits(m1[0])) and vals[at] == hv, n
        assert np.array_equal(bits(g[at][0]), bits(g1[0])) and np.array_equal(bits(g[at][1]), bits(g1[1])), n
        host, hmeans = ssim_amd.compute_msssimf_batch(pairs, 1.0, per_scale=True)
        assert np.array_equal(bits(host), bits(vals)) and np.array_equal(bits(hmeans), bits(means)) and np.array_equal(bits(means), bits(m)), n
        if n == 7:
            mods = [M.Model(a, b, 1.0) for a, b in pairs]
            for i in range(n):
                check_grad(g[i], mods[i], 1.0, g_out[i], 5, None, "batch of 7 [%d]" % i)


def test_host_batch_that_is_split_into_sub_batches():
    """70 pairs of 1920 x 1080 floats stage 1.16 GB and need 0.4 GB of pyramid: more than the 1 GB of scratch one sub-batch may hold."""
    from ssim_amd import synth
    distinct = []
    for seed in (1, 2, 3):
        a, b = synth.pair_numpy(1920, 1080, seed)
        distinct.append((a.astype(np.float32), b.astype(np.float32)))
    single = [ssim_amd.compute_msssimf(a, b, 255.0, per_scale=True) for a, b in distinct]
    got, means = ssim_amd.compute_msssimf_batch([distinct[i % 3] for i in range(70)], 255.0, per_scale=True)
    assert np.array_equal(bits(got), bits(np.array([single[i % 3][0] for i in range(70)], np.float32)))
    assert np.array_equal(bits(means), bits(np.array([single[i % 3][1] for i in range(70)])))


def test_device_batch_whose_backward_is_split_into_sub_batches(gpu_ctx):
    """140 pairs of 1920 x 1080 with dLoss/dA alone need 8.3 MB each of pyramid and coarse gradient planes: 129 pairs per GB of scratch,
    so the backward runs in two sub-batches (the forward, 5.6 MB a pair, in one).  Every pair reads the same two device images and
    writes a gradient plane of its own."""
    from ssim_amd import synth
    a, b = synth.pair_numpy(1920, 1080, 5)
    fa, fb = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
    h, w, n = 1080, 1920, 140
    one = DevicePairs(gpu_ctx, [(fa, fb)])
    want = one.grads(1.0, [0.7], want_b=False)[0][0]
    v1, m1 = one.forward(1.0)
    params = (ssim_amd.ParamsF * n)()
    for i in range(n):
        params[i] = one.params[0]
    vals, means, go = gpu_ctx.alloc(8 * n), gpu_ctx.alloc(80 * n), gpu_ctx.upload(np.full(n, 0.7, np.float32))
    out = gpu_ctx.alloc(4 * h * w * n)
    ga = (ssim_amd.GradF * n)()
    for i in range(n):
        ga[i] = ssim_amd.GradF(out.ptr + 4 * h * w * i, 1, w)
    gpu_ctx.enqueue_msssimf(params, n, 1.0, vals.ptr, means.ptr)
    gpu_ctx.enqueue_msssimf_grad(params, n, 1.0, means.ptr, go.ptr, ga, None)
    gpu_ctx.synchronize()
    v, m = vals.download(np.float64, (n,)), means.download(np.float64, (n, 5, 2))
    assert np.all(bits(v) == bits(v1)[0]) and all(np.array_equal(bits(m[i]), bits(m1[0])) for i in range(n))
    lib = gpu_ctx.lib
    for i in (0, 1, 127, 128, 129, 130, 139):
        plane = np.empty((h, w), np.float32)
        assert lib.rmgr_ssim_hip_memcpy_d2h(gpu_ctx.handle, plane.ctypes.data, out.ptr + 4 * h * w * i, plane.nbytes) == 0
        assert np.array_equal(bits(plane), bits(want)), i
    for x in (vals, means, go, out):
        x.free()
    one.free()


def test_views_with_negative_and_interleaved_steps(gpu_ctx, manifest):
    a, b = load_pair(manifest["bbb257x65_q50_ch1"])
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    v, m = ssim_amd.compute_msssimf(fa, fb, 255.0, per_scale=True)
    # negative steps: the flipped storage viewed back to front is the same image
    ra, rb = np.ascontiguousarray(fa[::-1, ::-1]), np.ascontiguousarray(fb[::-1, ::-1])
    v2, m2 = ssim_amd.compute_msssimf(ra[::-1, ::-1], rb[::-1, ::-1], 255.0, per_scale=True)
    assert v2 == v and np.array_equal(bits(m2), bits(m))
    # channel-interleaved storage: step = 3
    rgb_a, rgb_b = np.zeros(fa.shape + (3,), np.float32), np.zeros(fa.shape + (3,), np.float32)
    rgb_a[:, :, 1], rgb_b[:, :, 1] = fa, fb
    v3, m3 = ssim_amd.compute_msssimf(rgb_a[:, :, 1], rgb_b[:, :, 1], 255.0, per_scale=True)
    assert v3 == v and np.array_equal(bits(m3), bits(m))
    # the gradient: contiguous planes against step-3 inputs and step-2 gradient planes
    plain = DevicePairs(gpu_ctx, [(fa, fb)])
    g = plain.grads(255.0, [1.0])[0]
    assert np.array_equal(bits(plain.forward(255.0)[1][0]), bits(m))
    plain.free()
    inter = DevicePairs(gpu_ctx, [(fa, fb)], step=3)
    g3 = inter.grads(255.0, [1.0], gstep=2)[0]
    assert np.array_equal(bits(inter.forward(255.0)[1][0]), bits(m))
    inter.free()
    assert np.array_equal(bits(g3[0]), bits(g[0])) and np.array_equal(bits(g3[1]), bits(g[1]))
    # negative steps on the device: the flipped image addressed from its last sample
    h, w = fa.shape
    da, db = gpu_ctx.upload(ra), gpu_ctx.upload(rb)
    ps = (ssim_amd.ParamsF * 1)()
    last = 4 * (h * w - 1)
    ps[0] = ssim_amd.make_params_f(w, h, da.ptr + last, -1, -w, db.ptr + last, -1, -w)
    dv, dm = gpu_ctx.msssimf_device(ps, 1, 255.0, per_scale=True)
    assert dv[0] == v and np.array_equal(bits(dm[0]), bits(m))
    vals, means = gpu_ctx.alloc(8), gpu_ctx.alloc(80)
    go, out = gpu_ctx.upload(np.ones(1, np.float32)), gpu_ctx.alloc(4 * h * w)
    ga = (ssim_amd.GradF * 1)()
    ga[0] = ssim_amd.GradF(out.ptr + last, -1, -w)
    gpu_ctx.enqueue_msssimf(ps, 1, 255.0, vals.ptr, means.ptr)
    gpu_ctx.enqueue_msssimf_grad(ps, 1, 255.0, means.ptr, go.ptr, ga, None)
    gpu_ctx.synchronize()
    flipped = out.download(np.float32, (h, w))
    for x in (da, db, go, out, vals, means):
        x.free()
    assert np.array_equal(bits(flipped[::-1, ::-1]), bits(g[0]))


# ---- torch ----
# torch brings a HIP runtime of its own, which has to be the first one a process loads: the checks run in one child process
# (tests/tools/msssimf_torch_checks.py) that imports torch before the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "msssimf_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "msssimf_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["forward_and_backward_are_the_c_abi_bit_for_bit", "non_contiguous_slice_without_a_copy", "non_default_stream",
                                   "legacy_default_stream", "gradient_agrees_with_the_float64_model", "refusals_on_gpu_tensors",
                                   "training_step_memory_is_the_gradients_and_the_means"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
