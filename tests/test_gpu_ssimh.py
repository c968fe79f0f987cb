"""GPU: SSIM of float16 / bfloat16 samples and its gradient (rmgr_ssim_hip_enqueue_ssimh, rmgr_ssim_hip_compute_ssimh_device / _host,
rmgr_ssim_hip_enqueue_ssimh_grad, ssim_amd.torch_ops) held to the float32 path, bit for bit.

The contract (include/rmgr/ssim-hip.h): value, map and sums are those of ssimf on the samples widened to float32, and the gradient is
ssimf's float32 gradient of the widened planes rounded once, to nearest-even, into the samples' encoding.  Both widenings are exact, so
there is no tolerance here: the reference is always the existing ssimf path on the widened planes in the same process, and
tests/halfmodel.py's rounding (held to torch's by tests/test_ssimh_cpu.py).  NaN is compared as NaN, never by payload.  The one test
against the float64 model uses the as-stored golden pairs at range 255: integers 0..255 are exact in both encodings, so these are the
very planes ssimf_model.PX_TOL and G_TOL were measured on.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import halfmodel as HM
import ssimf_model as M
import ssim_amd
from conftest import ROOT, image_entries, load_pair
from ssimf_model import G_TOL, PX_TOL

pytestmark = pytest.mark.gpu

ENC = pytest.mark.parametrize("enc", HM.ENCODINGS)
SIZES = [(1, 1), (3, 5), (129, 127), (7, 300), (70, 150), (65, 257)]          # (H, W)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def encoded_pair(fa, fb, enc):
    """float32 planes -> (bit patterns of the encoding, the float32 planes those stand for)."""
    ua, ub = HM.round_to(fa, enc), HM.round_to(fb, enc)
    return (ua, ub), (HM.widen(ua, enc), HM.widen(ub, enc))


def random_pair(h, w, rng, enc):
    a = rng.random((h, w), dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal((h, w)).astype(np.float32), 0, 1).astype(np.float32)
    return encoded_pair(a, b, enc)


def host_ssimh(u, enc, r, want_map=True):
    a, st = HM.host_array(u[0], enc)
    b, _ = HM.host_array(u[1], enc)
    return ssim_amd.compute_ssimh(a, b, r, sample_type=st, want_map=want_map)


def check_forward(u, f, enc, r, what):
    """compute_ssimh of the bit patterns against compute_ssimf of the widened planes: value and map as bit patterns."""
    v, m = host_ssimh(u, enc, r)
    wv, wm = ssim_amd.compute_ssimf(f[0], f[1], r, want_map=True)
    assert HM.same_f32(np.array([v]), np.array([wv])), (what, enc, float(v), float(wv))
    assert HM.same_f32(m, wm), (what, enc)
    return v, m


class DevicePairs(object):
    """Pairs of one size in device memory, each image in a buffer of its own, samples `step` apart and `lead` elements into the buffer.
    kind "f": float32 planes (ParamsF, the reference path); else the encoding of uint16 bit patterns (Params16, the path under test)."""

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

    def sums(self, r):
        out = self.ctx.alloc(8 * self.n)
        if self.kind == "f":
            self.ctx.enqueue_ssimf(self.params, self.n, r, out.ptr)
        else:
            self.ctx.enqueue_ssimh(self.params, self.n, r, self.kind, out.ptr)
        self.ctx.synchronize()
        s = out.download(np.float64, (self.n,))
        out.free()
        return s

    def values(self, r):
        if self.kind == "f":
            return self.ctx.ssimf_device(self.params, self.n, r)
        return self.ctx.ssimh_device(self.params, self.n, r, self.kind)

    def grads(self, r, g_out, want_a=True, want_b=True, gstep=1, lead=0):
        """[(dLoss/dA or None, dLoss/dB or None)] per pair, in the pairs' sample type; gradient planes with samples gstep apart and
        `lead` elements into their buffer, everything but the gradient samples checked untouched."""
        ctx, n, h, w = self.ctx, self.n, self.h, self.w
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
            ctx.enqueue_ssimf_grad(self.params, n, r, go.ptr, arrs[0], arrs[1])
        else:
            ctx.enqueue_ssimh_grad(self.params, n, r, self.kind, go.ptr, arrs[0], arrs[1])
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
        for b in bufs[0] + bufs[1] + [go]:
            b.free()
        return out

    def free(self):
        for b in self.bufs:
            b.free()


def reference_grads(ctx, f_pairs, enc, r, g_out):
    """halfmodel.round(the ssimf gradient of the widened planes), per pair (dA, dB)."""
    ref = DevicePairs(ctx, f_pairs, "f")
    g32 = ref.grads(r, g_out)
    ref.free()
    return [(HM.round_to(ga, enc), HM.round_to(gb, enc)) for ga, gb in g32]


# ---- 1. forward, bit for bit ----

@ENC
def test_golden_fixtures_as_stored_and_in_the_unit_range(enc, manifest):
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        u, f = encoded_pair(a.astype(np.float32), b.astype(np.float32), enc)
        assert np.array_equal(f[0], a) and np.array_equal(f[1], b)               # integers 0..255 are exact in both encodings
        check_forward(u, f, enc, 255.0, n + "/stored")
        u, f = encoded_pair(a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255), enc)
        check_forward(u, f, enc, 1.0, n + "/unit")


@ENC
def test_small_and_odd_sizes(enc):
    rng = np.random.default_rng(7)
    for (h, w) in SIZES:
        u, f = random_pair(h, w, rng, enc)
        check_forward(u, f, enc, 1.0, "%dx%d" % (w, h))


@pytest.fixture(scope="module")
def synth_1080p():
    from ssim_amd import synth
    return [tuple(p.astype(np.float32) / np.float32(255) for p in synth.pair_numpy(1920, 1080, seed)) for seed in (1, 2, 3)]


@ENC
def test_1080p_value_and_sum(enc, gpu_ctx, synth_1080p):
    u, f = encoded_pair(synth_1080p[0][0], synth_1080p[0][1], enc)
    dh, df = DevicePairs(gpu_ctx, [u], enc), DevicePairs(gpu_ctx, [f], "f")
    sh, sf, vh, vf = dh.sums(1.0), df.sums(1.0), dh.values(1.0), df.values(1.0)
    dh.free()
    df.free()
    assert np.array_equal(bits(sh), bits(sf)) and np.array_equal(bits(vh), bits(vf)), (enc, sh, sf)
    assert 0.0 < float(vh[0]) < 1.0


# ---- 2. against the float64 model ----

@ENC
def test_golden_fixtures_as_stored_against_the_float64_model(enc, manifest):
    for n in image_entries(manifest):
        a, b = load_pair(manifest[n])
        u, f = encoded_pair(a.astype(np.float32), b.astype(np.float32), enc)
        v, m = host_ssimh(u, enc, 255.0)
        gv, gm = M.ssim(f[0], f[1], 255.0)
        dp = float(np.abs(m.astype(np.float64) - gm).max())
        print("%s %s: per-pixel %.3g, global %.3g" % (n, enc, dp, abs(float(v) - gv)))
        assert dp <= PX_TOL, (n, enc, dp)
        assert abs(float(v) - gv) <= G_TOL, (n, enc, float(v), gv)


# ---- 3. gradient, bit for bit ----

@ENC
def test_gradient_is_the_rounded_float32_gradient(enc, gpu_ctx):
    """gOut 1 (float16: mostly subnormal or zero -- the flush test), 0 (every pixel +-0), a negative one and W H (normal numbers); alone,
    A only, B only and both give the same bits."""
    rng = np.random.default_rng(13)
    subnormals = normals = 0
    for (h, w) in SIZES:
        pairs = [random_pair(h, w, rng, enc) for _ in range(4)]
        g_out = [1.0, 0.0, -0.6, float(w * h)]
        want = reference_grads(gpu_ctx, [f for _, f in pairs], enc, 1.0, g_out)
        dp = DevicePairs(gpu_ctx, [u for u, _ in pairs], enc)
        both = dp.grads(1.0, g_out)
        only_a = dp.grads(1.0, g_out, want_b=False)
        only_b = dp.grads(1.0, g_out, want_a=False)
        dp.free()
        single = DevicePairs(gpu_ctx, [pairs[2][0]], enc)
        alone = single.grads(1.0, [g_out[2]])[0]
        single.free()
        for i in range(4):
            for k in range(2):
                assert HM.same(both[i][k], want[i][k], enc), (enc, h, w, i, k)
            assert only_a[i][1] is None and only_b[i][0] is None
            assert np.array_equal(only_a[i][0], both[i][0]) and np.array_equal(only_b[i][1], both[i][1]), (enc, h, w, i)
        assert np.array_equal(alone[0], both[2][0]) and np.array_equal(alone[1], both[2][1]), (enc, h, w)
        assert np.all((both[1][0] & 0x7FFF) == 0) and np.all((both[1][1] & 0x7FFF) == 0)            # gOut = 0
        subnormals += int(HM.is_subnormal(both[0][0], enc).sum())
        n3 = both[3][0]
        normals += int((~HM.is_subnormal(n3, enc) & ((n3 & 0x7FFF) != 0)).sum())
    print("%s: %d subnormal gradient pixels at gOut = 1, %d normal ones at gOut = W H" % (enc, subnormals, normals))
    assert normals > 0
    if enc == HM.F16:
        assert subnormals > 0                          # the unscaled float16 gradient reaches below the normal range: kept, not flushed


# ---- 4. addressing ----

@ENC
def test_odd_element_offsets_interleaved_and_negative_steps(enc, gpu_ctx, manifest):
    a, b = load_pair(manifest["bbb257x65_q50_ch1"])                               # 257 columns: an odd width
    u, f = encoded_pair(a.astype(np.float32), b.astype(np.float32), enc)
    h, w = a.shape
    plain = DevicePairs(gpu_ctx, [u], enc)
    assert plain.params[0].imgA.topLeft % 4 == 0
    s, v, g = plain.sums(255.0), plain.values(255.0), plain.grads(255.0, [float(w * h)])[0]
    plain.free()
    want = reference_grads(gpu_ctx, [f], enc, 255.0, [float(w * h)])[0]
    assert HM.same(g[0], want[0], enc) and HM.same(g[1], want[1], enc)
    # a base pointer at an odd element offset: 2-byte but not 4-byte aligned, inputs and gradient planes, with the odd width
    odd = DevicePairs(gpu_ctx, [u], enc, lead=1)
    assert odd.params[0].imgA.topLeft % 4 == 2 and odd.params[0].imgB.topLeft % 4 == 2
    g1 = odd.grads(255.0, [float(w * h)], lead=1)[0]
    assert np.array_equal(bits(odd.sums(255.0)), bits(s)) and np.array_equal(bits(odd.values(255.0)), bits(v))
    # ... and the map of that pair, written on the device
    dmap = gpu_ctx.alloc(4 * h * w)
    odd.params[0].ssimMap, odd.params[0].ssimStep, odd.params[0].ssimStride = dmap.ptr, 1, w
    assert np.array_equal(bits(odd.values(255.0)), bits(v))
    m = dmap.download(np.float32, (h, w))
    dmap.free()
    odd.free()
    assert HM.same_f32(m, ssim_amd.compute_ssimf(f[0], f[1], 255.0, want_map=True)[1])
    assert np.array_equal(g1[0], g[0]) and np.array_equal(g1[1], g[1])
    # step-3 interleaved inputs (at an odd element offset again: lead 0 + step - 1 = 2, so lead 1 makes it 3) with step-2 gradient planes
    inter = DevicePairs(gpu_ctx, [u], enc, step=3, lead=1)
    g3 = inter.grads(255.0, [float(w * h)], gstep=2)[0]
    assert np.array_equal(bits(inter.sums(255.0)), bits(s)) and np.array_equal(bits(inter.values(255.0)), bits(v))
    inter.free()
    assert np.array_equal(g3[0], g[0]) and np.array_equal(g3[1], g[1])
    # host views: negative strides and a channel of an interleaved array
    hv, hm = host_ssimh(u, enc, 255.0)
    assert np.array_equal(bits(np.array([hv])), bits(v))
    ru = (np.ascontiguousarray(u[0][::-1, ::-1]), np.ascontiguousarray(u[1][::-1, ::-1]))
    v2, m2 = host_ssimh((ru[0][::-1, ::-1], ru[1][::-1, ::-1]), enc, 255.0)
    assert v2 == hv and np.array_equal(bits(m2), bits(hm))
    rgb = np.zeros((2,) + a.shape + (3,), np.uint16)
    rgb[0, :, :, 1], rgb[1, :, :, 1] = u
    v3, m3 = host_ssimh((rgb[0, :, :, 1], rgb[1, :, :, 1]), enc, 255.0)
    assert v3 == hv and np.array_equal(bits(m3), bits(hm))
    # negative steps on the device: the flipped image addressed from its last sample
    da, db = gpu_ctx.upload(ru[0]), gpu_ctx.upload(ru[1])
    ps = (ssim_amd.Params16 * 1)()
    last = 2 * (h * w - 1)
    ps[0] = ssim_amd.make_params16(w, h, da.ptr + last, -1, -w, db.ptr + last, -1, -w)
    go, out = gpu_ctx.upload(np.full(1, w * h, np.float32)), gpu_ctx.alloc(2 * h * w)
    ga = (ssim_amd.GradH * 1)()
    ga[0] = ssim_amd.GradH(out.ptr + last, -1, -w)
    gpu_ctx.enqueue_ssimh_grad(ps, 1, 255.0, enc, go.ptr, ga, None)
    gpu_ctx.synchronize()
    flipped = out.download(np.uint16, (h, w))
    assert np.array_equal(bits(gpu_ctx.ssimh_device(ps, 1, 255.0, enc)), bits(v))
    for x in (da, db, go, out):
        x.free()
    assert np.array_equal(flipped[::-1, ::-1], g[0])


# ---- 5. determinism ----

def einstein_pairs(manifest, enc):
    out = []
    for n in image_entries(manifest):
        if n.startswith("einstein_") and n != "einstein_einstein":
            a, b = load_pair(manifest[n])
            out.append(encoded_pair(a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255), enc)[0])
    return out


def host_batch(pairs, enc, r):
    if enc == HM.F16:
        return ssim_amd.compute_ssimh_batch([(a.view(np.float16), b.view(np.float16)) for a, b in pairs], r)
    return ssim_amd.compute_ssimh_batch(pairs, r, sample_type=enc)


@ENC
def test_same_bits_alone_in_batches_and_on_every_call(enc, gpu_ctx, manifest):
    pool = einstein_pairs(manifest, enc)
    pair = pool[0]
    h, w = pair[0].shape
    v1, m1 = host_ssimh(pair, enc, 1.0)
    alone = DevicePairs(gpu_ctx, [pair], enc)
    s1 = alone.sums(1.0)
    g1 = alone.grads(1.0, [0.5 * w * h])[0]
    assert np.array_equal(bits(alone.sums(1.0)), bits(s1))                               # repeated calls
    g1b = alone.grads(1.0, [0.5 * w * h])[0]
    assert np.array_equal(g1b[0], g1[0]) and np.array_equal(g1b[1], g1[1])
    assert np.float32(s1[0] / (float(w) * float(h))) == v1
    assert float(alone.values(1.0)[0]) == float(v1)                                      # every entry point
    alone.free()
    for n in (2, 7, 33):
        at = n // 2
        pairs = [pool[(i + 1) % len(pool)] for i in range(n)]
        pairs[at] = pair
        dp = DevicePairs(gpu_ctx, pairs, enc)
        s = dp.sums(1.0)
        g = dp.grads(1.0, [(0.25 * (i - at) + 0.5) * w * h for i in range(n)])
        vals = dp.values(1.0)
        dp.free()
        assert bits(s)[at] == bits(s1)[0] and vals[at] == v1, n
        assert np.array_equal(g[at][0], g1[0]) and np.array_equal(g[at][1], g1[1]), n
        assert np.array_equal(bits(host_batch(pairs, enc, 1.0)), bits(vals)), n
    v2, m2 = host_ssimh(pair, enc, 1.0)
    assert v2 == v1 and np.array_equal(bits(m1), bits(m2))


@ENC
def test_host_batch_that_is_split_into_sub_batches(enc, synth_1080p):
    """140 references to three distinct pairs of 1920 x 1080 stage 1.16 GB of 2-byte samples: more than the 1 GB of scratch one
    sub-batch may hold."""
    distinct = [encoded_pair(a, b, enc)[0] for a, b in synth_1080p]
    single = [host_ssimh(p, enc, 1.0, want_map=False)[0] for p in distinct]
    got = host_batch([distinct[i % 3] for i in range(140)], enc, 1.0)
    assert np.array_equal(bits(got), bits(np.array([single[i % 3] for i in range(140)], np.float32)))


# ---- 6. special values ----

@ENC
def test_nan_at_a_centre_position_spoils_its_121_windows(enc, gpu_ctx):
    rng = np.random.default_rng(9)
    u, _ = random_pair(64, 300, rng, enc)
    u[0][31, 64] = 0x7E00 if enc == HM.F16 else 0x7FC0       # NaN at the first strip column's centre position
    f = (HM.widen(u[0], enc), HM.widen(u[1], enc))
    assert np.isnan(f[0][31, 64]) and np.isnan(f[0]).sum() == 1
    v, m = check_forward(u, f, enc, 1.0, "nan")
    bad = np.isnan(m)
    assert np.isnan(v) and bad[26:37, 59:70].all() and bad.sum() == 121
    dp = DevicePairs(gpu_ctx, [u], enc)
    g = dp.grads(1.0, [float(64 * 300)])[0]
    dp.free()
    want = reference_grads(gpu_ctx, [f], enc, 1.0, [float(64 * 300)])[0]
    assert HM.same(g[0], want[0], enc) and HM.same(g[1], want[1], enc) and HM.is_nan(g[0], enc).any() and not HM.is_nan(g[0], enc).all()


@ENC
def test_the_largest_values_are_used_as_stored_and_the_centre_falls_back_to_zero(enc, gpu_ctx):
    rng = np.random.default_rng(10)
    u, _ = random_pair(40, 300, rng, enc)
    big = 0x7BFF if enc == HM.F16 else 0x7F61                # 65504; about 2.99e38
    u[0][19, 64] = big                                       # a centre position: above the range, so that strip column's centre is 0
    u[1][19, 192] = big | 0x8000
    u[1][5, 250] = big
    f = (HM.widen(u[0], enc), HM.widen(u[1], enc))
    assert np.isfinite(f[0][19, 64]) and f[0][19, 64] == (65504.0 if enc == HM.F16 else np.float32(2.0 ** 127 * (1 + 0x61 / 128.0)))
    v, m = check_forward(u, f, enc, 1.0, "large")
    assert np.isfinite(m[:, 100:120]).all()                  # columns no window of a large value reaches
    dp = DevicePairs(gpu_ctx, [u], enc)
    g = dp.grads(1.0, [float(40 * 300)])[0]
    dp.free()
    want = reference_grads(gpu_ctx, [f], enc, 1.0, [float(40 * 300)])[0]
    assert HM.same(g[0], want[0], enc) and HM.same(g[1], want[1], enc)


def test_a_float16_plane_of_subnormals(gpu_ctx):
    rng = np.random.default_rng(11)
    ua = rng.integers(1, 0x400, (50, 140)).astype(np.uint16)
    ub = rng.integers(1, 0x400, (50, 140)).astype(np.uint16) | np.uint16(0x8000) * (rng.random((50, 140)) < 0.3).astype(np.uint16)
    assert HM.is_subnormal(ua, HM.F16).all() and HM.is_subnormal(ub, HM.F16).all()
    f = (HM.widen(ua, HM.F16), HM.widen(ub, HM.F16))
    assert np.all(f[0] > 0) and np.abs(f[1]).min() >= 2.0 ** -24
    r = float(2.0 ** -14)                                    # the span of the subnormals
    v, m = check_forward((ua, ub), f, HM.F16, r, "subnormals")
    assert np.ptp(m) > 0.1                                   # flushed samples would make both planes 0 and every pixel 1
    dp = DevicePairs(gpu_ctx, [(ua, ub)], HM.F16)
    g = dp.grads(r, [1e-3])[0]
    dp.free()
    want = reference_grads(gpu_ctx, [f], HM.F16, r, [1e-3])[0]
    assert HM.same(g[0], want[0], HM.F16) and HM.same(g[1], want[1], HM.F16)


# ---- 7. torch ----
# torch brings a HIP runtime of its own, which has to be the first one a process loads: the checks run in one child process
# (tests/tools/ssimh_torch_checks.py) that imports torch before the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "ssimh_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "ssimh_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["forward_and_backward_are_the_c_abi_bit_for_bit", "non_contiguous_slice_without_a_copy",
                                   "non_default_and_legacy_default_stream", "a_scaled_loss_is_rounded_once", "autocast_conv_feeds_the_loss",
                                   "memory_is_the_gradient_tensor_and_nothing_else"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
