"""GPU: SSIM of float32 samples and its gradient (rmgr_ssim_hip_enqueue_ssimf, rmgr_ssim_hip_compute_ssimf_device / _host,
rmgr_ssim_hip_enqueue_ssimf_grad, ssim_amd.torch_ops) against the float64 definition (tests/ssimf_model.py), and their determinism.

Bounds.  Measured, not estimated: an fp32 emulation of the kernels' arithmetic (ssimf_model.emulate_fp32) lands within 2.38e-4 per
pixel, 1.17e-6 globally and 8.37e-5 of the plane's largest float64 gradient magnitude of the model on every golden pair in three forms
(/ 255 at range 1, as stored at range 255, scaled by a non-integer factor to range 1000), and leaves max|grad| * W * H * R = 3.65e-4 on
the pair of identical images, whose exact gradient is 0 (tests/test_ssimf_cpu.py pins these figures).  The asserted bounds are about
twice that: PX_TOL = 5e-4, G_TOL = 2.5e-6, GRAD_TOL = 1.7e-4, IDENT_TOL = 7.5e-4.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ssimf_model as M
import ssim_amd
from conftest import ROOT, image_entries, load_pair
from ssimf_model import G_TOL, GRAD_TOL, IDENT_TOL, PX_TOL, forms

pytestmark = pytest.mark.gpu

G16_TOL = 1.3e-6            # the ssim16 path's global bound (tests/test_gpu_ssim16.py)
SMALL = [(1, 1), (3, 5), (129, 127), (7, 300)]          # (H, W): 1 x 1, 5 x 3, 127 x 129 and 300 x 7 as W x H


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if np.asarray(x).dtype == np.float32 else np.uint64)


def check_forward(a, b, r, what, every=1):
    v, m = ssim_amd.compute_ssimf(a, b, r, want_map=True)
    gv, gm = M.ssim(a, b, r)
    dp = float(np.abs(m.astype(np.float64) - gm)[::every, ::every].max())
    print("%s: per-pixel %.3g, global %.3g" % (what, dp, abs(float(v) - gv)))
    assert dp <= PX_TOL, (what, dp)
    assert abs(float(v) - gv) <= G_TOL, (what, float(v), gv)
    return v, m


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

    def sums(self, r):
        out = self.ctx.alloc(8 * self.n)
        self.ctx.enqueue_ssimf(self.params, self.n, r, out.ptr)
        self.ctx.synchronize()
        s = out.download(np.float64, (self.n,))
        out.free()
        return s

    def grads(self, r, g_out, want_a=True, want_b=True, gstep=1):
        """[(dLoss/dA or None, dLoss/dB or None)] per pair; gradient planes with samples gstep apart, the gaps checked untouched."""
        ctx, n, h, w = self.ctx, self.n, self.h, self.w
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
        ctx.enqueue_ssimf_grad(self.params, n, r, go.ptr, arrs[0], arrs[1])
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
        for b in bufs[0] + bufs[1] + [go]:
            b.free()
        return out

    def free(self):
        for b in self.bufs:
            b.free()


def check_grad(got, a, b, r, g_out, what, identical=False):
    ga, gb = M.grad(a, b, r, g_out)
    for name, g, want in (("dA", got[0], ga), ("dB", got[1], gb)):
        if g is None:
            continue
        assert g.shape == want.shape and np.all(np.isfinite(g)), (what, name)
        if g_out == 0:
            assert np.all(g == 0), (what, name)
        elif identical:
            e = float(np.abs(g).max()) * g.size * r / abs(g_out)
            print("%s %s: identical images, max|grad| W H R = %.3g" % (what, name, e))
            assert e <= IDENT_TOL, (what, name, e)
        else:
            e = float(np.abs(g - want).max() / np.abs(want).max())
            print("%s %s: %.3g of max|grad|" % (what, name, e))
            assert e <= GRAD_TOL, (what, name, e)


# ---- forward ----

def test_golden_fixtures_in_three_forms(manifest):
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        for form, fa, fb, r in forms(a, b):
            check_forward(fa, fb, r, "%s/%s" % (n, form))


def test_small_sizes_down_to_one_pixel():
    rng = np.random.default_rng(7)
    for (h, w) in SMALL:
        for r in (1.0, 255.0):
            a, b = random_pair(h, w, rng, r)
            check_forward(a, b, r, "%dx%d/%g" % (w, h, r))


def test_1080p_and_4096_square():
    from ssim_amd import synth
    for (w, h) in ((1920, 1080), (4096, 4096)):
        a, b = synth.pair_numpy(w, h)
        fa, fb = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
        check_forward(fa, fb, 1.0, "synth %dx%d" % (w, h), every=3 if w == 4096 else 1)


def test_integer_valued_floats_agree_with_ssim16_at_depth_8(manifest):
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        vf, _ = ssim_amd.compute_ssimf(a.astype(np.float32), b.astype(np.float32), 255.0)
        v16, _ = ssim_amd.compute_ssim16(a.astype(np.uint16), b.astype(np.uint16), 8)
        assert abs(float(vf) - float(v16)) <= G_TOL + G16_TOL, (n, float(vf), float(v16))


def test_nan_and_values_outside_the_range_propagate_locally():
    rng = np.random.default_rng(9)
    a, b = random_pair(64, 300, rng)
    a[31, 64] = np.nan                                   # the first strip column's centre position
    b[10, 200] = 7.5                                     # above the range: used as stored
    v, m = ssim_amd.compute_ssimf(a, b, 1.0, want_map=True)
    bad = np.isnan(m)
    assert np.isnan(v) and bad[26:37, 59:70].all() and bad.sum() == 121          # the 11 x 11 windows that hold the NaN, nothing else
    assert np.all(np.abs(m[~bad]) <= 1.0 + 1e-5)


# ---- gradient ----

def test_gradient_of_golden_fixtures_in_three_forms(gpu_ctx, manifest):
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        for form, fa, fb, r in forms(a, b):
            dp = DevicePairs(gpu_ctx, [(fa, fb)])
            got = dp.grads(r, [1.0])[0]
            dp.free()
            check_grad(got, fa, fb, r, 1.0, "%s/%s" % (n, form), identical=np.array_equal(a, b))


def test_gradient_alone_together_and_with_differing_grad_out(gpu_ctx):
    """gradA alone, gradB alone and both together give the same bits; gOut differs per image, with a 0 and a negative one."""
    rng = np.random.default_rng(13)
    for (h, w) in SMALL + [(70, 150)]:
        pairs = [random_pair(h, w, rng) for _ in range(4)]
        g_out = [1.0, 0.0, -0.6, 2.5]
        dp = DevicePairs(gpu_ctx, pairs)
        both = dp.grads(1.0, g_out)
        only_a = dp.grads(1.0, g_out, want_b=False)
        only_b = dp.grads(1.0, g_out, want_a=False)
        dp.free()
        for i, (a, b) in enumerate(pairs):
            check_grad(both[i], a, b, 1.0, g_out[i], "%dx%d[%d]" % (w, h, i))
            assert only_a[i][1] is None and only_b[i][0] is None
            assert np.array_equal(bits(only_a[i][0]), bits(both[i][0])) and np.array_equal(bits(only_b[i][1]), bits(both[i][1])), (h, w, i)


def test_gradient_at_1080p(gpu_ctx):
    from ssim_amd import synth
    a, b = synth.pair_numpy(1920, 1080)
    fa, fb = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
    dp = DevicePairs(gpu_ctx, [(fa, fb)])
    got = dp.grads(1.0, [-1.0])[0]
    dp.free()
    check_grad(got, fa, fb, 1.0, -1.0, "synth 1920x1080")


# ---- determinism ----

def einstein_pairs(manifest):
    out = []
    for n in image_entries(manifest):
        if n.startswith("einstein_") and n != "einstein_einstein":
            a, b = load_pair(manifest[n])
            out.append((a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)))
    return out


def test_same_bits_alone_in_batches_and_on_every_call(gpu_ctx, manifest):
    pool = einstein_pairs(manifest)
    pair = pool[0]
    v1, m1 = ssim_amd.compute_ssimf(pair[0], pair[1], 1.0, want_map=True)
    alone = DevicePairs(gpu_ctx, [pair])
    s1 = alone.sums(1.0)
    g1 = alone.grads(1.0, [0.5])[0]
    assert np.array_equal(bits(alone.sums(1.0)), bits(s1))                               # repeated calls
    g1b = alone.grads(1.0, [0.5])[0]
    assert np.array_equal(bits(g1b[0]), bits(g1[0])) and np.array_equal(bits(g1b[1]), bits(g1[1]))
    assert np.float32(s1[0] / (float(pair[0].shape[1]) * float(pair[0].shape[0]))) == v1
    assert float(gpu_ctx.ssimf_device(alone.params, 1, 1.0)[0]) == float(v1)            # every entry point
    alone.free()
    for n in (2, 7, 33):
        at = n // 2
        pairs = [pool[(i + 1) % len(pool)] for i in range(n)]
        pairs[at] = pair
        dp = DevicePairs(gpu_ctx, pairs)
        s = dp.sums(1.0)
        g = dp.grads(1.0, [0.25 * (i - at) + 0.5 for i in range(n)])
        vals = gpu_ctx.ssimf_device(dp.params, n, 1.0)
        dp.free()
        assert bits(s)[at] == bits(s1)[0] and vals[at] == v1, n
        assert np.array_equal(bits(g[at][0]), bits(g1[0])) and np.array_equal(bits(g[at][1]), bits(g1[1])), n
        host = ssim_amd.compute_ssimf_batch(pairs, 1.0)
        assert np.array_equal(bits(host), bits(vals)), n
    v2, m2 = ssim_amd.compute_ssimf(pair[0], pair[1], 1.0, want_map=True)
    assert v2 == v1 and np.array_equal(bits(m1), bits(m2))


def test_host_batch_that_is_split_into_sub_batches(manifest):
    """70 pairs of 1920 x 1080 floats stage 1.16 GB: more than the 1 GB of scratch one sub-batch may hold."""
    from ssim_amd import synth
    distinct = []
    for seed in (1, 2, 3):
        a, b = synth.pair_numpy(1920, 1080, seed)
        distinct.append((a.astype(np.float32), b.astype(np.float32)))
    single = [ssim_amd.compute_ssimf(a, b, 255.0)[0] for a, b in distinct]
    got = ssim_amd.compute_ssimf_batch([distinct[i % 3] for i in range(70)], 255.0)
    assert np.array_equal(bits(got), bits(np.array([single[i % 3] for i in range(70)], np.float32)))


def test_views_with_negative_and_interleaved_steps(gpu_ctx, manifest):
    a, b = load_pair(manifest["bbb257x65_q50_ch1"])
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    v, m = ssim_amd.compute_ssimf(fa, fb, 255.0, want_map=True)
    # negative steps: the flipped storage viewed back to front is the same image
    ra, rb = np.ascontiguousarray(fa[::-1, ::-1]), np.ascontiguousarray(fb[::-1, ::-1])
    v2, m2 = ssim_amd.compute_ssimf(ra[::-1, ::-1], rb[::-1, ::-1], 255.0, want_map=True)
    assert v2 == v and np.array_equal(bits(m2), bits(m))
    # channel-interleaved storage: step = 3
    rgb_a, rgb_b = np.zeros(fa.shape + (3,), np.float32), np.zeros(fa.shape + (3,), np.float32)
    rgb_a[:, :, 1], rgb_b[:, :, 1] = fa, fb
    v3, m3 = ssim_amd.compute_ssimf(rgb_a[:, :, 1], rgb_b[:, :, 1], 255.0, want_map=True)
    assert v3 == v and np.array_equal(bits(m3), bits(m))
    # the gradient: contiguous planes against step-3 inputs and step-2 gradient planes
    plain = DevicePairs(gpu_ctx, [(fa, fb)])
    g = plain.grads(255.0, [1.0])[0]
    assert plain.sums(255.0)[0] / (257.0 * 65.0) == pytest.approx(float(v), abs=1e-7)
    plain.free()
    inter = DevicePairs(gpu_ctx, [(fa, fb)], step=3)
    g3 = inter.grads(255.0, [1.0], gstep=2)[0]
    assert np.float32(inter.sums(255.0)[0] / (257.0 * 65.0)) == v
    inter.free()
    assert np.array_equal(bits(g3[0]), bits(g[0])) and np.array_equal(bits(g3[1]), bits(g[1]))
    # negative steps on the device: the flipped image addressed from its last sample
    h, w = fa.shape
    da, db = gpu_ctx.upload(ra), gpu_ctx.upload(rb)
    ps = (ssim_amd.ParamsF * 1)()
    last = 4 * (h * w - 1)
    ps[0] = ssim_amd.make_params_f(w, h, da.ptr + last, -1, -w, db.ptr + last, -1, -w)
    go, out = gpu_ctx.upload(np.ones(1, np.float32)), gpu_ctx.alloc(4 * h * w)
    ga = (ssim_amd.GradF * 1)()
    ga[0] = ssim_amd.GradF(out.ptr + last, -1, -w)
    gpu_ctx.enqueue_ssimf_grad(ps, 1, 255.0, go.ptr, ga, None)
    gpu_ctx.synchronize()
    flipped = out.download(np.float32, (h, w))
    assert gpu_ctx.ssimf_device(ps, 1, 255.0)[0] == v
    for x in (da, db, go, out):
        x.free()
    assert np.array_equal(bits(flipped[::-1, ::-1]), bits(g[0]))


# ---- torch ----
# torch brings a HIP runtime of its own, which has to be the first one a process loads: the checks run in one child process
# (tests/tools/ssimf_torch_checks.py) that imports torch before the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "ssimf_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "ssimf_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["forward_and_backward_are_the_c_abi_bit_for_bit", "non_contiguous_slice_without_a_copy", "non_default_stream",
                                   "gradient_ascent_raises_ssim_at_every_step", "gradient_agrees_with_a_float64_conv2d_restatement"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
