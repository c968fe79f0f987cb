"""GPU: multi-scale SSIM of float16 / bfloat16 samples and its gradient (rmgr_ssim_hip_enqueue_msssimh, rmgr_ssim_hip_compute_msssimh_device /
_host, rmgr_ssim_hip_enqueue_msssimh_grad, ssim_amd.torch_ops.ms_ssim_amp) held to the float32 multi-scale path, bit for bit.

The contract (include/rmgr/ssim-hip.h): the value and every per-scale mean are those of msssimf on the samples widened to float32, and the
gradient is the float32 value msssimf's gradient would store at scale 0, rounded once, to nearest-even, into the samples' encoding.  Both
widenings are exact, so there is no tolerance here: the reference is always the existing msssimf path on the widened planes in the same
process, and tests/halfmodel.py's rounding (held to torch's by tests/test_ssimh_cpu.py).  NaN is compared as NaN, never by payload.  The
one test against the float64 model uses the as-stored golden pairs at range 255: integers 0..255 are exact in both encodings, so these
are planes msssimf_model.VALUE_TOL and MEAN_TOL were measured on.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import content_classes as C
import halfmodel as HM
import msssimf_model as M
import ssim_amd
from conftest import ROOT, image_entries, load_pair
from msssimf_model import MEAN_TOL, VALUE_TOL

pytestmark = pytest.mark.gpu

ENC = pytest.mark.parametrize("enc", HM.ENCODINGS)
SIZES = [(1, 1), (3, 5), (17, 33), (65, 257), (129, 127), (7, 300)]     # (H, W): odd at every scale, several strip columns and tiles
CONFIGS = [(5, None)] + [(m, (1.0 / m,) * m) for m in range(1, 9)]      # Wang's five; uniform weights at 1 .. 8 scales (1: the LAST form at scale 0)
ZERO_AT_0 = (3, (0.0, 0.5, 0.5))                                        # k_0 == 0: scale 0 stores the rounded upstream


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def same_f64(got, want):
    """float64 arrays with the same bit patterns, NaN compared as NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(bits(got[~gn]), bits(want[~wn]))


def encoded_pair(fa, fb, enc):
    """float32 planes -> (bit patterns of the encoding, the float32 planes those stand for)."""
    ua, ub = HM.round_to(fa, enc), HM.round_to(fb, enc)
    return (ua, ub), (HM.widen(ua, enc), HM.widen(ub, enc))


def random_pair(h, w, rng, enc):
    a = rng.random((h, w), dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal((h, w)).astype(np.float32), 0, 1).astype(np.float32)
    return encoded_pair(a, b, enc)


def host_arrays(u, enc):
    """(a, b, sample_type) as ssim_amd.compute_msssimh takes these bit patterns."""
    a, st = HM.host_array(u[0], enc)
    return a, HM.host_array(u[1], enc)[0], st


class DevicePairs(object):
    """Pairs of one size in device memory, each image in a buffer of its own, samples `step` apart and `lead` elements into the buffer.
    kind "f": float32 planes (ParamsF, msssimf: the reference path); else the encoding of uint16 bit patterns (Params16, msssimh)."""

    def __init__(self, ctx, pairs, kind, step=1, lead=0):
        self.ctx, self.n, self.kind = ctx, len(pairs), kind
        self.h, self.w = pairs[0][0].shape
        self.dt, self.es = (np.float32, 4) if kind == "f" else (np.uint16, 2)
        self.bufs = []
        self.params = ((ssim_amd.ParamsF if kind == "f" else ssim_amd.Params16) * self.n)()
        make = ssim_amd.make_params_f if kind == "f" else ssim_amd.make_params16
        for i, (a, b) in enumerate(pairs):
            d = []
            for img in (a, b):
                store = np.zeros(lead + self.h * self.w * step, self.dt)
                store[lead:].reshape(self.h, self.w, step)[:, :, step - 1] = img
                d.append(ctx.upload(store))
            self.bufs += d
            off = self.es * (lead + step - 1)
            self.params[i] = make(self.w, self.h, d[0].ptr + off, step, self.w * step, d[1].ptr + off, step, self.w * step)

    def forward(self, r, scales=5, weights=None, keep=False):
        """(values float64 (n,), means float64 (n, scales, 2)) through the enqueue entry; keep: also the device buffer of the means."""
        vals, means = self.ctx.alloc(8 * self.n), self.ctx.alloc(16 * self.n * scales)
        if self.kind == "f":
            self.ctx.enqueue_msssimf(self.params, self.n, r, vals.ptr, means.ptr, scales, weights)
        else:
            self.ctx.enqueue_msssimh(self.params, self.n, r, self.kind, vals.ptr, means.ptr, scales, weights)
        self.ctx.synchronize()
        v, m = vals.download(np.float64, (self.n,)), means.download(np.float64, (self.n, scales, 2))
        vals.free()
        if keep:
            return v, m, means
        means.free()
        return v, m

    def device(self, r, scales=5, weights=None):
        if self.kind == "f":
            return self.ctx.msssimf_device(self.params, self.n, r, scales, weights, per_scale=True)
        return self.ctx.msssimh_device(self.params, self.n, r, self.kind, scales, weights, per_scale=True)

    def grads(self, r, g_out, scales=5, weights=None, want_a=True, want_b=True, gstep=1, lead=0, means=None):
        """[(dLoss/dA or None, dLoss/dB or None)] per pair, forward then backward, in the pairs' sample type; gradient planes with samples
        gstep apart and `lead` elements into their buffer, everything but the gradient samples checked untouched.  means: a float64
        (n, scales, 2) array handed to the backward in place of this forward's."""
        ctx, n, h, w = self.ctx, self.n, self.h, self.w
        if means is None:
            _, _, means = self.forward(r, scales, weights, keep=True)
        else:
            means = np.ascontiguousarray(means, np.float64)
            assert means.shape == (n, scales, 2)
            means = ctx.upload(means)
        go = ctx.upload(np.asarray(g_out, np.float32))
        mark = self.dt(-777.0) if self.kind == "f" else np.uint16(0xABCD)
        fill = np.full(lead + h * w * gstep, mark, self.dt)
        cls = ssim_amd.GradF if self.kind == "f" else ssim_amd.GradH
        arrs, bufs = [None, None], [[], []]
        for k, want in enumerate((want_a, want_b)):
            if not want:
                continue
            arrs[k] = (cls * n)()
            for i in range(n):
                buf = ctx.upload(fill)
                bufs[k].append(buf)
                arrs[k][i] = cls(buf.ptr + self.es * lead, gstep, w * gstep)
        if self.kind == "f":
            ctx.enqueue_msssimf_grad(self.params, n, r, means.ptr, go.ptr, arrs[0], arrs[1], scales, weights)
        else:
            ctx.enqueue_msssimh_grad(self.params, n, r, self.kind, means.ptr, go.ptr, arrs[0], arrs[1], scales, weights)
        ctx.synchronize()
        out = []
        for i in range(n):
            pair = []
            for k in range(2):
                if arrs[k] is None:
                    pair.append(None)
                    continue
                raw = bufs[k][i].download(self.dt, (lead + h * w * gstep,))
                g = raw[lead:].reshape(h, w, gstep)
                assert np.all(bits(raw[:lead]) == bits(fill[:1])[0]) and np.all(bits(g[:, :, 1:]) == bits(fill[:1])[0])
                pair.append(np.ascontiguousarray(g[:, :, 0]))
            out.append(tuple(pair))
        for b in bufs[0] + bufs[1] + [go, means]:
            b.free()
        return out

    def free(self):
        for b in self.bufs:
            b.free()


def handed_means(means, clean):
    """What the backward is handed: None -- the forward's own means --, or, `clean` given, the forward's means with those of every pair
    that has a NaN among them replaced by `clean`, a finite (scales, 2) array (NaN means make every k_s NaN)."""
    if clean is None:
        return None
    out = np.array(means, np.float64)
    for i in range(len(out)):
        if np.isnan(out[i]).any():
            out[i] = clean
    return out


def reference(ctx, f_pairs, enc, r, g_out, scales=5, weights=None, clean=None):
    """msssimf on the widened planes: (values, means, [(round(dA), round(dB))], the float32 gradients themselves)."""
    ref = DevicePairs(ctx, f_pairs, "f")
    v, m = ref.forward(r, scales, weights)
    g32 = ref.grads(r, g_out, scales, weights, means=handed_means(m, clean))
    ref.free()
    return v, m, [(HM.round_to(ga, enc), HM.round_to(gb, enc)) for ga, gb in g32], g32


def check_pairs(ctx, u_pairs, f_pairs, enc, r, g_out, scales, weights, what, clean=None):
    """Value, means, dA alone, dB alone and both of the bit patterns against the reference.  Returns (both, float32 reference gradients).
    clean: see handed_means; both paths are handed the same means."""
    wv, wm, want, g32 = reference(ctx, f_pairs, enc, r, g_out, scales, weights, clean)
    dp = DevicePairs(ctx, u_pairs, enc)
    v, m = dp.forward(r, scales, weights)
    handed = handed_means(wm, clean)
    both = dp.grads(r, g_out, scales, weights, means=handed)
    only_a = dp.grads(r, g_out, scales, weights, want_b=False, means=handed)
    only_b = dp.grads(r, g_out, scales, weights, want_a=False, means=handed)
    dp.free()
    assert same_f64(v, wv) and same_f64(m, wm), (what, enc, scales, v, wv)
    for i in range(len(u_pairs)):
        for k in range(2):
            assert HM.same(both[i][k], want[i][k], enc), (what, enc, scales, i, k)
        assert only_a[i][1] is None and only_b[i][0] is None
        assert HM.same(only_a[i][0], both[i][0], enc) and HM.same(only_b[i][1], both[i][1], enc), (what, enc, scales, i)
    return both, g32


# ---- 1. odd sizes at every scale, every number of scales, one gradient or both ----

@ENC
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_small_and_odd_sizes_at_every_number_of_scales(enc, size, gpu_ctx):
    h, w = size
    rng = np.random.default_rng(7 + h)
    u, f = random_pair(h, w, rng, enc)
    g_out = [-0.75 * w * h]                                  # keeps the float16 gradient in the normal range
    nonzero = 0
    for scales, wts in CONFIGS + [ZERO_AT_0]:
        both, g32 = check_pairs(gpu_ctx, [u], [f], enc, 1.0, g_out, scales, wts, "%dx%d" % (w, h))
        if (scales, wts) == ZERO_AT_0 and min(h, w) >= 3:
            # k_0 == 0: what scale 0 stores is 0.0f + the coarser scales' gradient, and that is not nothing
            assert np.any(g32[0][0] != 0) and np.any((both[0][0] & 0x7FFF) != 0), (enc, size)
        nonzero += int(np.count_nonzero(both[0][0] & 0x7FFF))
    assert nonzero > 0 or h * w == 1


@ENC
def test_tall_strip_with_32_row_cells_at_scale_0_and_8_row_cells_below(enc, gpu_ctx):
    """2115 x 9 (H x W) at 3 scales: 32-row cells and several cell batches at scale 0 (H >= 2048), 8-row cells at 1058 and 529 rows, a
    short last cell at every scale."""
    rng = np.random.default_rng(21)
    u, f = random_pair(2115, 9, rng, enc)
    check_pairs(gpu_ctx, [u], [f], enc, 1.0, [0.5 * 2115 * 9], 3, (0.3, 0.3, 0.4), "tall")


# ---- 2. determinism ----

def einstein_pairs(manifest, enc, count=5):
    out = []
    for n in image_entries(manifest):
        if n.startswith("einstein_") and n != "einstein_einstein":
            a, b = load_pair(manifest[n])
            out.append(encoded_pair(a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255), enc))
    assert len(out) >= count
    return [u for u, _ in out[:count]], [f for _, f in out[:count]]


def host_batch(pairs, enc, r):
    if enc == HM.F16:
        return ssim_amd.compute_msssimh_batch([(a.view(np.float16), b.view(np.float16)) for a, b in pairs], r, per_scale=True)
    return ssim_amd.compute_msssimh_batch(pairs, r, sample_type=enc, per_scale=True)


@ENC
def test_same_bits_alone_in_a_batch_in_a_split_batch_through_every_entry_and_on_every_call(enc, gpu_ctx, manifest):
    us, fs = einstein_pairs(manifest, enc)
    h, w = us[0][0].shape
    g_out = [(0.25 * i + 0.5) * w * h for i in range(5)]
    wv, wm, want, _ = reference(gpu_ctx, fs, enc, 1.0, g_out)
    batch = DevicePairs(gpu_ctx, us, enc)
    v, m = batch.forward(1.0)
    g = batch.grads(1.0, g_out)
    assert same_f64(v, wv) and same_f64(m, wm)
    v2, m2 = batch.forward(1.0)                                                           # a second call
    g2 = batch.grads(1.0, g_out)
    dv, dm = batch.device(1.0)                                                            # every entry point
    batch.free()
    hv, hm = host_batch(us, enc, 1.0)
    assert np.array_equal(bits(v2), bits(v)) and np.array_equal(bits(m2), bits(m))
    assert np.array_equal(bits(dv), bits(v.astype(np.float32))) and np.array_equal(bits(dm), bits(m))
    assert np.array_equal(bits(hv), bits(dv)) and np.array_equal(bits(hm), bits(m))
    for i in range(5):
        for k in range(2):
            assert HM.same(g[i][k], want[i][k], enc) and np.array_equal(g2[i][k], g[i][k]), (enc, i, k)
    # alone, and in a batch split 2 + 3
    for lo, hi in ((0, 2), (2, 5)) + tuple((i, i + 1) for i in range(5)):
        part = DevicePairs(gpu_ctx, us[lo:hi], enc)
        pv, pm = part.forward(1.0)
        pg = part.grads(1.0, g_out[lo:hi])
        pdv, _ = part.device(1.0)
        part.free()
        assert np.array_equal(bits(pv), bits(v[lo:hi])) and np.array_equal(bits(pm), bits(m[lo:hi])) and np.array_equal(bits(pdv), bits(dv[lo:hi])), (lo, hi)
        for i in range(lo, hi):
            assert np.array_equal(pg[i - lo][0], g[i][0]) and np.array_equal(pg[i - lo][1], g[i][1]), (lo, hi, i)
        if hi - lo == 1:
            a, b, st = host_arrays(us[lo], enc)
            sv, sm = ssim_amd.compute_msssimh(a, b, 1.0, sample_type=st, per_scale=True)
            assert bits(np.array([sv]))[0] == bits(dv)[lo] and np.array_equal(bits(sm), bits(m[lo]))


# ---- 3. views ----

@ENC
def test_negative_interleaved_and_odd_offset_views(enc, gpu_ctx, manifest):
    a, b = load_pair(manifest["bbb257x65_q50_ch1"])                               # 257 columns: an odd width
    u, f = encoded_pair(a.astype(np.float32), b.astype(np.float32), enc)
    h, w = a.shape
    g_out = [float(w * h)]
    wv, wm, want, _ = reference(gpu_ctx, [f], enc, 255.0, g_out)
    plain = DevicePairs(gpu_ctx, [u], enc)
    v, m = plain.forward(255.0)
    g = plain.grads(255.0, g_out)[0]
    plain.free()
    assert same_f64(v, wv) and same_f64(m, wm) and HM.same(g[0], want[0][0], enc) and HM.same(g[1], want[0][1], enc)
    # a channel of an interleaved 3-channel buffer (step 3) that starts at an odd 2-byte offset, with step-2 gradient planes one
    # element into their buffers; the markers around the gradient samples are checked by grads()
    inter = DevicePairs(gpu_ctx, [u], enc, step=3, lead=1)
    assert inter.params[0].imgA.topLeft % 4 == 2 and inter.params[0].imgB.topLeft % 4 == 2
    v3, m3 = inter.forward(255.0)
    g3 = inter.grads(255.0, g_out, gstep=2, lead=1)[0]
    inter.free()
    assert np.array_equal(bits(v3), bits(v)) and np.array_equal(bits(m3), bits(m))
    assert np.array_equal(g3[0], g[0]) and np.array_equal(g3[1], g[1])
    # host views: negative strides and a channel of an interleaved array
    ha, hb, st = host_arrays(u, enc)
    hv, hm = ssim_amd.compute_msssimh(ha, hb, 255.0, sample_type=st, per_scale=True)
    assert np.float32(v[0]) == hv and np.array_equal(bits(hm), bits(m[0]))
    ru = (np.ascontiguousarray(u[0][::-1, ::-1]), np.ascontiguousarray(u[1][::-1, ::-1]))
    ha, hb, st = host_arrays((ru[0][::-1, ::-1], ru[1][::-1, ::-1]), enc)
    v2, m2 = ssim_amd.compute_msssimh(ha, hb, 255.0, sample_type=st, per_scale=True)
    assert v2 == hv and np.array_equal(bits(m2), bits(hm))
    rgb = np.zeros((2,) + a.shape + (3,), np.uint16)
    rgb[0, :, :, 1], rgb[1, :, :, 1] = u
    ha, hb, st = host_arrays((rgb[0, :, :, 1], rgb[1, :, :, 1]), enc)
    v4, m4 = ssim_amd.compute_msssimh(ha, hb, 255.0, sample_type=st, per_scale=True)
    assert v4 == hv and np.array_equal(bits(m4), bits(hm))
    # negative step and stride on the device: the flipped image addressed from its last sample, and the gradient plane likewise
    da, db = gpu_ctx.upload(ru[0]), gpu_ctx.upload(ru[1])
    ps = (ssim_amd.Params16 * 1)()
    last = 2 * (h * w - 1)
    ps[0] = ssim_amd.make_params16(w, h, da.ptr + last, -1, -w, db.ptr + last, -1, -w)
    dv, dm = gpu_ctx.msssimh_device(ps, 1, 255.0, enc, per_scale=True)
    assert dv[0] == hv and np.array_equal(bits(dm[0]), bits(hm))
    vals, means = gpu_ctx.alloc(8), gpu_ctx.alloc(80)
    go, out = gpu_ctx.upload(np.asarray(g_out, np.float32)), gpu_ctx.alloc(2 * h * w)
    ga = (ssim_amd.GradH * 1)()
    ga[0] = ssim_amd.GradH(out.ptr + last, -1, -w)
    gpu_ctx.enqueue_msssimh(ps, 1, 255.0, enc, vals.ptr, means.ptr)
    gpu_ctx.enqueue_msssimh_grad(ps, 1, 255.0, enc, means.ptr, go.ptr, ga, None)
    gpu_ctx.synchronize()
    flipped = out.download(np.uint16, (h, w))
    for x in (da, db, go, out, vals, means):
        x.free()
    assert np.array_equal(flipped[::-1, ::-1], g[0])


@ENC
@pytest.mark.parametrize("sign", [1, -1], ids=["forwards", "backwards"])
def test_64_bit_form_with_samples_far_apart(enc, sign, gpu_ctx):
    """One 9 x 5 (H x W) pair at 2 scales with samples 2^22 apart -- the first step fitsh_narrow() refuses --, forwards and with a negative
    step: the bits of the dense call.  One volume of W columns 2^22 elements apart, rows one element apart: A in rows 0 .., B in rows
    16 .., dLoss/dA in rows 32 .., dLoss/dB in rows 48 .. of every column; everything else is filler and must stay untouched."""
    h, w, far = 9, 5, 1 << 22
    rng = np.random.default_rng(33)
    u, f = random_pair(h, w, rng, enc)
    g_out, scales, wts = [float(w * h)], 2, (0.4, 0.6)
    dense = DevicePairs(gpu_ctx, [u], enc)
    v, m = dense.forward(1.0, scales, wts)
    g = dense.grads(1.0, g_out, scales, wts)[0]
    dense.free()
    _, _, want, _ = reference(gpu_ctx, [f], enc, 1.0, g_out, scales, wts)
    assert HM.same(g[0], want[0][0], enc) and HM.same(g[1], want[0][1], enc)
    vol = np.full(w * far, 0x7FC0, np.uint16)                 # a NaN in both encodings
    cols = vol.reshape(w, far)
    expect = vol.copy().reshape(w, far)
    for x in range(w):
        c = x if sign > 0 else w - 1 - x
        for k, plane in enumerate(u):
            cols[c, 16 * k:16 * k + h] = plane[:, x]
            expect[c, 16 * k:16 * k + h] = plane[:, x]
        for k in range(2):
            expect[c, 32 + 16 * k:32 + 16 * k + h] = g[k][:, x]
    dvol = gpu_ctx.upload(vol)
    first = 0 if sign > 0 else (w - 1) * far                  # the element of column x = 0
    ps = (ssim_amd.Params16 * 1)()
    ps[0] = ssim_amd.make_params16(w, h, dvol.ptr + 2 * first, sign * far, 1, dvol.ptr + 2 * (first + 16), sign * far, 1)
    ga, gb = (ssim_amd.GradH * 1)(), (ssim_amd.GradH * 1)()
    ga[0], gb[0] = ssim_amd.GradH(dvol.ptr + 2 * (first + 32), sign * far, 1), ssim_amd.GradH(dvol.ptr + 2 * (first + 48), sign * far, 1)
    vals, means, go = gpu_ctx.alloc(8), gpu_ctx.alloc(16 * scales), gpu_ctx.upload(np.asarray(g_out, np.float32))
    gpu_ctx.enqueue_msssimh(ps, 1, 1.0, enc, vals.ptr, means.ptr, scales, wts)
    gpu_ctx.enqueue_msssimh_grad(ps, 1, 1.0, enc, means.ptr, go.ptr, ga, gb, scales, wts)
    gpu_ctx.synchronize()
    fv, fm = vals.download(np.float64, (1,)), means.download(np.float64, (1, scales, 2))
    got = dvol.download(np.uint16, (w, far))
    for x in (dvol, vals, means, go):
        x.free()
    assert np.array_equal(bits(fv), bits(v)) and np.array_equal(bits(fm), bits(m))
    assert np.array_equal(got, expect)


# ---- 4. special values ----

def test_a_float16_plane_of_subnormals(gpu_ctx):
    rng = np.random.default_rng(11)
    ua = rng.integers(1, 0x400, (50, 140)).astype(np.uint16)
    ub = rng.integers(1, 0x400, (50, 140)).astype(np.uint16) | np.uint16(0x8000) * (rng.random((50, 140)) < 0.3).astype(np.uint16)
    assert HM.is_subnormal(ua, HM.F16).all() and HM.is_subnormal(ub, HM.F16).all()
    f = (HM.widen(ua, HM.F16), HM.widen(ub, HM.F16))
    r = float(2.0 ** -14)                                    # the span of the subnormals
    check_pairs(gpu_ctx, [(ua, ub)], [f], HM.F16, r, [1e-3], 3, (0.3, 0.3, 0.4), "subnormals")
    v = ssim_amd.compute_msssimh(ua.view(np.float16), ub.view(np.float16), r, scales=3, weights=(0.3, 0.3, 0.4))
    assert float(v) < 0.9                                    # flushed samples would make both planes 0 and the value 1


@ENC
def test_one_nan_sample(enc, gpu_ctx):
    rng = np.random.default_rng(9)
    u, _ = random_pair(64, 300, rng, enc)
    u[0][31, 70] = 0x7E00 if enc == HM.F16 else 0x7FC0
    f = (HM.widen(u[0], enc), HM.widen(u[1], enc))
    assert np.isnan(f[0]).sum() == 1
    a, b, st = host_arrays(u, enc)
    v, means = ssim_amd.compute_msssimh(a, b, 1.0, sample_type=st, per_scale=True)
    assert np.isnan(v) and np.isnan(means[:, 0]).all()
    # the gradient is NaN exactly where msssimf's is (HM.same compares the NaN positions); with the forward's NaN means every k_s is
    # NaN, so finite means are handed to the backward instead: those of the pair without the NaN
    clean = (u[0].copy(), u[1])
    clean[0][31, 70] = 0
    cf = (HM.widen(clean[0], enc), f[1])
    h, w = 64, 300
    planes = {}
    for kind, bad, good in (("f", f, cf), (enc, u, clean)):
        dg, dbad = DevicePairs(gpu_ctx, [good], kind), DevicePairs(gpu_ctx, [bad], kind)
        _, _, means_dev = dg.forward(1.0, keep=True)
        go = gpu_ctx.upload(np.full(1, w * h, np.float32))
        es, cls = (4, ssim_amd.GradF) if kind == "f" else (2, ssim_amd.GradH)
        out = gpu_ctx.alloc(es * h * w)
        ga = (cls * 1)()
        ga[0] = cls(out.ptr, 1, w)
        if kind == "f":
            gpu_ctx.enqueue_msssimf_grad(dbad.params, 1, 1.0, means_dev.ptr, go.ptr, ga, None)
        else:
            gpu_ctx.enqueue_msssimh_grad(dbad.params, 1, 1.0, enc, means_dev.ptr, go.ptr, ga, None)
        gpu_ctx.synchronize()
        planes[kind] = out.download(np.float32 if kind == "f" else np.uint16, (h, w))
        for x in (means_dev, go, out):
            x.free()
        dg.free()
        dbad.free()
    nan = HM.is_nan(planes[enc], enc)
    assert HM.same(planes[enc], HM.round_to(planes["f"], enc), enc) and nan.any() and not nan.all()
    assert np.array_equal(nan, np.isnan(planes["f"]))
    # and with the forward's own means: NaN coefficients, NaN everywhere, as msssimf
    check_pairs(gpu_ctx, [u], [f], enc, 1.0, [float(w * h)], 5, None, "nan")


@ENC
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_sample_content_and_a_bad_sample_at_the_centre_of_every_scale(enc, gpu_ctx):
    """The catalogue of tests/content_classes.py on the grid the 16-bit encodings hold (exact=True) as planes of 300 x 40, and the eight
    planes of tests/test_gpu_msssimf_content.py with a 1e15 (Inf in float16), a NaN or an Inf at the centre of a strip column of one
    scale, on A or on B; 4 uniform scales.  Forward and gradients have the bits of msssimf on the widened planes.  Where the forward's
    means are NaN the backward of both paths is handed the clean base pair's means, as in test_one_nan_sample: the gradient is then NaN
    in part of the plane, not all of it.  The 18 classes of range 1 and the eight planes go in one launch, neighbours differing in
    content; the other ranges one by one."""
    shape, scales, wts = M.CONTENT_SHAPE, M.CONTENT_SCALES, M.CONTENT_WEIGHTS
    h, w = shape
    classes = C.plane_classes(shape, exact=True)
    base = tuple((np.round(x * np.float32(128)) / np.float32(128)).astype(np.float32) for x in M.base_pair())
    assert np.array_equal(C.named(classes, "negative")[1], -base[0]) and np.array_equal(C.named(classes, "negative")[2], -base[1])
    planted = []
    for s, pos in enumerate(M.CONTENT_POSITIONS):
        assert M.centre_scales(shape, pos, scales) == [s]
        for k, side in enumerate("AB"):
            a, b = base[0].copy(), base[1].copy()
            (a if side == "A" else b)[pos] = (C.HUGE, np.nan, np.inf)[(2 * s + k) % 3]
            planted.append(("centre of scale %d (%s)" % (s, side), a, b))
    unit = [(c[0], c[1], c[2]) for c in classes if c[3] == 1.0]
    entries = [e for pair in zip(unit, planted) for e in pair] + unit[len(planted):]
    assert len(entries) == 26
    (cu, cf) = encoded_pair(base[0], base[1], enc)
    assert np.array_equal(cf[0], base[0]) and np.array_equal(cf[1], base[1])                     # the grid is exact in both encodings
    dp = DevicePairs(gpu_ctx, [cf], "f")
    _, clean = dp.forward(1.0, scales, wts)
    dp.free()
    clean = clean[0]
    assert np.all(np.isfinite(clean))
    enc_pairs = [encoded_pair(a, b, enc) for _, a, b in entries]
    us, fs = [u for u, _ in enc_pairs], [f for _, f in enc_pairs]
    huge = HM.widen(HM.round_to(np.full(1, C.HUGE, np.float32), enc), enc)[0]
    assert np.isinf(huge) if enc == HM.F16 else (np.isfinite(huge) and huge > 9e14)
    g_out = [(-0.75 + 0.25 * i) * w * h for i in range(len(entries))]                            # differs per pair; one is 0
    both, g32 = check_pairs(gpu_ctx, us, fs, enc, 1.0, g_out, scales, wts, "content", clean=clean)
    partly = 0
    for i, (name, _, _) in enumerate(entries):
        if g_out[i] != 0 and not np.all(np.isfinite(fs[i][0]) & np.isfinite(fs[i][1])):
            nan = HM.is_nan(both[i][0], enc)
            assert nan.any() and not nan.all() and np.array_equal(nan, np.isnan(g32[i][0])), (name, enc)
            partly += 1
    assert partly >= 7, partly
    for name, a, b, r, _ in classes:
        if r != 1.0:
            u, f = encoded_pair(a, b, enc)
            check_pairs(gpu_ctx, [u], [f], enc, r, [-0.75 * w * h * r], scales, wts, name, clean=clean)


def test_float16_overflows_to_inf_exactly_where_the_rounded_float32_gradient_does(gpu_ctx, manifest):
    us, fs = einstein_pairs(manifest, HM.F16, 1)
    both, g32 = check_pairs(gpu_ctx, us, fs, HM.F16, 1.0, [1e30], 5, None, "overflow")
    inf = (both[0][0] & 0x7FFF) == 0x7C00
    assert inf.any() and np.array_equal(inf, np.abs(g32[0][0]) >= 65520.0) and np.isfinite(g32[0][0]).all()


@ENC
def test_a_loss_scale_is_applied_before_the_single_rounding(enc, gpu_ctx, manifest):
    """gradOut = 65536 (a GradScaler's scale) gives round(65536 g), not 65536 round(g): in float16 the unscaled gradient of a 256 x 256
    pair is subnormal or zero and has lost bits that the scaled one keeps."""
    us, fs = einstein_pairs(manifest, enc, 1)
    scaled, _ = check_pairs(gpu_ctx, us, fs, enc, 1.0, [65536.0], 5, None, "scaled")
    dp = DevicePairs(gpu_ctx, us, enc)
    unscaled = dp.grads(1.0, [1.0])[0]
    dp.free()
    twice = HM.round_to(HM.widen(unscaled[0], enc) * np.float32(65536.0), enc)                 # 65536 round(g)
    differ = int((twice != scaled[0][0]).sum())
    print("%s: %d of %d pixels differ from 65536 * round(g)" % (enc, differ, twice.size))
    if enc == HM.F16:                                        # bfloat16 has float32's exponent range: a power of two commutes with its rounding
        assert differ > 0


@ENC
def test_relu_pair_has_an_all_zero_gradient(enc, gpu_ctx, manifest):
    a, _ = load_pair(manifest["einstein_jpg"])
    (ua, _), (fa, _) = encoded_pair(a.astype(np.float32) / np.float32(255), a.astype(np.float32) / np.float32(255), enc)
    (ub, _), (fb, _) = encoded_pair(np.float32(1) - fa, fa, enc)
    h, w = a.shape
    both, _ = check_pairs(gpu_ctx, [(ua, ub)], [(fa, fb)], enc, 1.0, [float(w * h)], 5, None, "relu")
    dp = DevicePairs(gpu_ctx, [(ua, ub)], enc)
    v, m = dp.forward(1.0)
    dp.free()
    assert bits(v)[0] == 0 and np.all(m[0, :, 0] < 0), (v, m)
    assert not both[0][0].any() and not both[0][1].any()                   # +0 everywhere, bit for bit: no NaN, no -0


# ---- 5. against the float64 model ----

@ENC
def test_golden_fixtures_as_stored_against_the_float64_model(enc, manifest):
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        u, f = encoded_pair(a.astype(np.float32), b.astype(np.float32), enc)
        assert np.array_equal(f[0], a) and np.array_equal(f[1], b)               # integers 0..255 are exact in both encodings
        ha, hb, st = host_arrays(u, enc)
        v, means = ssim_amd.compute_msssimh(ha, hb, 255.0, sample_type=st, per_scale=True)
        mv, mm = M.Model(f[0], f[1], 255.0).msssim(5, None)
        dv, dm = abs(float(v) - mv), float(np.abs(means - mm).max())
        print("%s %s: value %.3g, per-scale means %.3g" % (n, enc, dv, dm))
        assert dv <= VALUE_TOL, (n, enc, float(v), mv)
        assert dm <= MEAN_TOL, (n, enc, means, mm)


# ---- 6. torch ----
# torch brings a HIP runtime of its own, which has to be the first one a process loads: the checks run in one child process
# (tests/tools/msssimh_torch_checks.py) that imports torch before the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "msssimh_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "msssimh_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["forward_and_backward_are_the_float32_path_bit_for_bit", "non_contiguous_channel_slice_without_a_copy",
                                   "non_default_stream", "autocast_conv_feeds_the_loss", "training_step_memory_is_the_16_bit_gradient"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
