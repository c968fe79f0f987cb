"""GPU: the gradient of the SSIM map for a per-pixel upstream gradient (rmgr_ssim_hip_enqueue_ssimf_map_grad, _enqueue_ssimh_map_grad,
ssim_amd.torch_ops.ssim_map): held to the existing gradient kernels bit for bit where the definitions coincide, to the float64
definition (tests/ssimw_model.py) elsewhere, and deterministic.

Bounds.  Measured, not estimated: an fp32 emulation of the kernel's arithmetic (ssimw_model.emulate_fp32_map_grad) lands within 1.06e-4 of
the plane's largest float64 gradient magnitude on every golden pair in three forms under three weight planes, and leaves
max|grad| * R / max|gmap| = 8.94e-5 where the exact gradient is 0 (tests/test_ssimw_cpu.py pins these figures).  The asserted bounds are
about twice that: WGRAD_TOL = 2.1e-4, WIDENT_TOL = 1.8e-4.

Sizes are W x H.  130 x 70 crosses a strip column (the centre changes at x = 128) and spans 5 x 3 gradient tiles.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import halfmodel as HM
import ssimw_model as MW
import ssim_amd
from conftest import ROOT, load_pair
from ssimf_model import forms
from ssimw_model import WGRAD_TOL, WIDENT_TOL

pytestmark = pytest.mark.gpu

G_OUT = -0.75
FILL32, FILL16 = np.float32(-777.0), np.uint16(0x5A5A)


def random_pair(w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.random((h, w), dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal((h, w)).astype(np.float32), 0, 1).astype(np.float32)
    return a, b


def pair_of(manifest, w, h):
    """1 x 1 ... 130 x 70: seeded random pairs; 257 x 65 and 255 x 63: the golden pairs, / 255."""
    name = {(257, 65): "bbb257x65_q50_ch1", (255, 63): "bbb255x63_q50_ch1"}.get((w, h))
    if name is None:
        return random_pair(w, h, 100 * w + h)
    a, b = load_pair(manifest[name])
    return a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)


class Plane(object):
    """One H x W plane in device memory in a layout of its own: samples `step` apart (the plane is the last channel of an interleaved
    buffer), and, when flipped, stored back to front and addressed from its last sample with a negative step and stride."""

    def __init__(self, ctx, arr, step=1, flip=False, fill=None):
        self.h, self.w = arr.shape
        self.step, self.flip, self.dtype = step, flip, arr.dtype
        host = np.zeros((self.h, self.w, step), arr.dtype) if fill is None else np.full((self.h, self.w, step), fill, arr.dtype)
        host[:, :, step - 1] = arr[::-1, ::-1] if flip else arr
        self.fill = fill
        self.buf = ctx.upload(host)
        es = arr.dtype.itemsize
        first = es * (step - 1)
        if flip:
            self.ptr, self.dstep, self.dstride = self.buf.ptr + first + es * step * (self.h * self.w - 1), -step, -self.w * step
        else:
            self.ptr, self.dstep, self.dstride = self.buf.ptr + first, step, self.w * step

    def read(self):
        """The plane as stored now; the gaps between its samples must hold what they were filled with."""
        host = self.buf.download(self.dtype, (self.h, self.w, self.step))
        if self.fill is not None and self.step > 1:
            assert np.all(host[:, :, :self.step - 1] == self.fill)
        p = host[:, :, self.step - 1]
        return np.ascontiguousarray(p[::-1, ::-1] if self.flip else p)

    def free(self):
        self.buf.free()


def run(ctx, pairs, maps, r, which=3, enc=None, step=1, flip=False, scalar=None, uniform=None):
    """dLoss/dA and / or dLoss/dB of `pairs` ([(a, b)], float32, or uint16 bit patterns with enc) through the entry under test, for the
    planes `maps`; or, with scalar = [g], for one float per pair delivered with step = stride = 0; or, with uniform = [gOut], through
    the EXISTING entry (rmgr_ssim_hip_enqueue_ssimf_grad / _ssimh_grad).  Samples, weights and gradient planes all use the layout (step,
    flip).  Returns [(ga or None, gb or None)]."""
    n = len(pairs)
    h, w = pairs[0][0].shape
    half = enc is not None
    dt, fill = (np.uint16, FILL16) if half else (np.float32, FILL32)
    made = []

    def plane(arr, **kw):
        p = Plane(ctx, arr, **kw)
        made.append(p)
        return p
    ps = ((ssim_amd.Params16 if half else ssim_amd.ParamsF) * n)()
    make = ssim_amd.make_params16 if half else ssim_amd.make_params_f
    for i, (a, b) in enumerate(pairs):
        pa, pb = plane(np.asarray(a, dt), step=step, flip=flip), plane(np.asarray(b, dt), step=step, flip=flip)
        ps[i] = make(w, h, pa.ptr, pa.dstep, pa.dstride, pb.ptr, pb.dstep, pb.dstride)
    cls = ssim_amd.GradH if half else ssim_amd.GradF
    arrs, outs = [None, None], [[], []]
    for k in range(2):
        if which & (1 << k):
            arrs[k] = (cls * n)()
            for i in range(n):
                g = plane(np.full((h, w), fill, dt), step=step, flip=flip, fill=fill)
                outs[k].append(g)
                arrs[k][i] = cls(g.ptr, g.dstep, g.dstride)
    if uniform is not None:
        go = ctx.upload(np.asarray(uniform, np.float32))
        if half:
            ctx.enqueue_ssimh_grad(ps, n, r, enc, go.ptr, arrs[0], arrs[1])
        else:
            ctx.enqueue_ssimf_grad(ps, n, r, go.ptr, arrs[0], arrs[1])
    else:
        ms = (ssim_amd.GradOutF * n)()
        if scalar is not None:
            go = ctx.upload(np.asarray(scalar, np.float32))
            for i in range(n):
                ms[i] = ssim_amd.GradOutF(go.ptr + 4 * i, 0, 0)
        else:
            go = None
            for i in range(n):
                m = plane(np.asarray(maps[i], np.float32), step=step, flip=flip)
                ms[i] = ssim_amd.GradOutF(m.ptr, m.dstep, m.dstride)
        if half:
            ctx.enqueue_ssimh_map_grad(ps, n, r, enc, ms, arrs[0], arrs[1])
        else:
            ctx.enqueue_ssimf_map_grad(ps, n, r, ms, arrs[0], arrs[1])
    ctx.synchronize()
    res = [tuple(outs[k][i].read() if arrs[k] is not None else None for k in range(2)) for i in range(n)]
    for p in made:
        p.free()
    if go is not None:
        go.free()
    return res


def same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.uint16),
                                                                        y.view(np.uint32 if y.dtype == np.float32 else np.uint16))


# ---- the identity clause: a constant plane of float(gOut / (W H)) gives the existing kernels' bits ----

@pytest.mark.parametrize("w,h", [(1, 1), (5, 1), (3, 5), (33, 31), (40, 48), (130, 70), (257, 65)])
@pytest.mark.parametrize("delivery", ["plane", "stride0"])
def test_constant_plane_has_the_bits_of_ssimf_grad(gpu_ctx, manifest, w, h, delivery):
    pair = pair_of(manifest, w, h)
    k = MW.constant_plane(G_OUT, h, w)
    assert k[0, 0] == np.float32(float(np.float32(G_OUT)) / (float(w) * float(h)))
    for which in (1, 2, 3):
        want = run(gpu_ctx, [pair], None, 1.0, which, uniform=[G_OUT])[0]
        got = run(gpu_ctx, [pair], [k], 1.0, which) if delivery == "plane" else run(gpu_ctx, [pair], None, 1.0, which, scalar=[k[0, 0]])
        for g, wt in zip(got[0], want):
            assert (g is None) == (wt is None)
            if g is not None:
                assert same(g, wt) and np.abs(g).max() > 0, (w, h, which, delivery)


@pytest.mark.parametrize("w,h", [(33, 31), (130, 70)])
@pytest.mark.parametrize("enc", HM.ENCODINGS)
def test_constant_plane_has_the_bits_of_ssimh_grad(gpu_ctx, manifest, w, h, enc):
    a, b = pair_of(manifest, w, h)
    pair = (HM.round_to(a, enc), HM.round_to(b, enc))
    k = MW.constant_plane(G_OUT, h, w)
    for which in (1, 2, 3):
        want = run(gpu_ctx, [pair], None, 1.0, which, enc=enc, uniform=[G_OUT])[0]
        got = run(gpu_ctx, [pair], [k], 1.0, which, enc=enc)[0]
        zero = run(gpu_ctx, [pair], None, 1.0, which, enc=enc, scalar=[k[0, 0]])[0]
        for g, z, wt in zip(got, zero, want):
            if wt is not None:
                assert same(g, wt) and same(z, wt) and (g & 0x7FFF).max() > 0, (w, h, which, enc)


# ---- accuracy against the float64 definition ----

def weight_planes(h, w, seed):
    """The three planes of ssimw_model.weight_planes, then one-hot weights on the image's corners, on the two sides of the first tile
    corner, and on the last column of the first strip column (clipped into the plane, duplicates dropped)."""
    out = list(MW.weight_planes(h, w, seed))
    seen = {(min(31, h - 1), min(31, w - 1))}
    for (y, x) in ((0, 0), (h - 1, w - 1), (32, 32), (h // 2, 127)):
        y, x = min(y, h - 1), min(x, w - 1)
        if (y, x) not in seen:
            seen.add((y, x))
            out.append(("one-hot(%d,%d)" % (y, x), MW.one_hot(h, w, y, x)))
    return out


def check_against_the_model(got, a, b, r, gmap, what):
    want = MW.grad_map(a, b, r, gmap)
    for name, g, wt in (("dA", got[0], want[0]), ("dB", got[1], want[1])):
        assert g.shape == wt.shape and np.all(np.isfinite(g)), (what, name)
        if MW.is_null(wt, gmap, r):
            e = float(np.abs(g).max()) * r / float(np.abs(gmap).max())
            print("%s %s: exact gradient 0, max|grad| R / max|gmap| = %.3g" % (what, name, e))
            assert e <= WIDENT_TOL, (what, name, e)
        else:
            e = float(np.abs(g - wt).max() / np.abs(wt).max())
            print("%s %s: %.3g of max|grad|" % (what, name, e))
            assert e <= WGRAD_TOL, (what, name, e)


@pytest.mark.parametrize("w,h", [(255, 63), (257, 65)])
def test_golden_pairs_in_three_forms_against_the_model(gpu_ctx, manifest, w, h):
    a8, b8 = load_pair(manifest["bbb%dx%d_q50_ch1" % (w, h)])
    for form, fa, fb, r in forms(a8, b8):
        planes = weight_planes(h, w, seed=w)
        got = run(gpu_ctx, [(fa, fb)] * len(planes), [p for _, p in planes], r)
        for (name, p), g in zip(planes, got):
            check_against_the_model(g, fa, fb, r, p, "%dx%d/%s/%s" % (w, h, form, name))


@pytest.mark.parametrize("w,h", [(33, 31), (130, 70)])
def test_random_pairs_against_the_model_and_16_bit_against_float32(gpu_ctx, manifest, w, h):
    a, b = pair_of(manifest, w, h)
    planes = weight_planes(h, w, seed=w)
    got = run(gpu_ctx, [(a, b)] * len(planes), [p for _, p in planes], 1.0)
    for (name, p), g in zip(planes, got):
        check_against_the_model(g, a, b, 1.0, p, "%dx%d/%s" % (w, h, name))
    # 16-bit samples: the float32 result on the widened planes, rounded once
    for enc in HM.ENCODINGS:
        ua, ub = HM.round_to(a, enc), HM.round_to(b, enc)
        wide = run(gpu_ctx, [(HM.widen(ua, enc), HM.widen(ub, enc))] * len(planes), [p for _, p in planes], 1.0)
        half = run(gpu_ctx, [(ua, ub)] * len(planes), [p for _, p in planes], 1.0, enc=enc)
        for (name, p), g32, g16 in zip(planes, wide, half):
            for k in range(2):
                assert HM.same(g16[k], HM.round_to(g32[k], enc), enc), (w, h, enc, name, k)
                assert (g16[k] & 0x7FFF).max() > 0, (w, h, enc, name, k)


def test_zero_weights_give_a_zero_gradient(gpu_ctx, manifest):
    a, b = pair_of(manifest, 130, 70)
    zero = np.zeros((70, 130), np.float32)
    ga, gb = run(gpu_ctx, [(a, b)], [zero], 1.0)[0]
    assert np.all(ga == 0) and np.all(gb == 0)
    for enc in HM.ENCODINGS:
        ga, gb = run(gpu_ctx, [(HM.round_to(a, enc), HM.round_to(b, enc))], [zero], 1.0, enc=enc)[0]
        assert np.all((ga & 0x7FFF) == 0) and np.all((gb & 0x7FFF) == 0), enc


# ---- determinism ----

def test_same_bits_alone_in_a_batch_through_views_and_with_one_gradient_or_both(gpu_ctx, manifest):
    w, h = 130, 70
    pair = pair_of(manifest, w, h)
    others = [random_pair(w, h, 5), random_pair(w, h, 6)]
    planes = [p for _, p in MW.weight_planes(h, w, seed=9)]
    alone = run(gpu_ctx, [pair], [planes[0]], 1.0)[0]
    assert np.abs(alone[0]).max() > 0 and np.abs(alone[1]).max() > 0
    for at in range(3):                                  # anywhere in a batch of 3 whose weight planes differ
        pairs = [others[0], others[1]]
        maps = [planes[1], planes[2]]
        pairs.insert(at, pair)
        maps.insert(at, planes[0])
        got = run(gpu_ctx, pairs, maps, 1.0)[at]
        assert same(got[0], alone[0]) and same(got[1], alone[1]), at
    # samples, weights and gradient planes interleaved three apart, stored back to front behind negative steps, and both
    for step, flip in ((3, False), (1, True), (2, True)):
        got = run(gpu_ctx, [pair], [planes[0]], 1.0, step=step, flip=flip)[0]
        assert same(got[0], alone[0]) and same(got[1], alone[1]), (step, flip)
    only_a = run(gpu_ctx, [pair], [planes[0]], 1.0, which=1)[0]
    only_b = run(gpu_ctx, [pair], [planes[0]], 1.0, which=2)[0]
    assert only_a[1] is None and only_b[0] is None and same(only_a[0], alone[0]) and same(only_b[1], alone[1])
    again = run(gpu_ctx, [pair], [planes[0]], 1.0)[0]
    assert same(again[0], alone[0]) and same(again[1], alone[1])
    for enc in HM.ENCODINGS:                             # 16-bit: batch position, a view, one gradient or both
        up = (HM.round_to(pair[0], enc), HM.round_to(pair[1], enc))
        uo = (HM.round_to(others[0][0], enc), HM.round_to(others[0][1], enc))
        one = run(gpu_ctx, [up], [planes[0]], 1.0, enc=enc)[0]
        got = run(gpu_ctx, [uo, up], [planes[1], planes[0]], 1.0, enc=enc, step=3, flip=True)[1]
        assert same(got[0], one[0]) and same(got[1], one[1]), enc
        assert same(run(gpu_ctx, [up], [planes[0]], 1.0, which=2, enc=enc)[0][1], one[1]), enc


# ---- torch ----
# torch brings a HIP runtime of its own, which has to be the first one a process loads: the checks run in one child process
# (tests/tools/ssimw_torch_checks.py) that imports torch before the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "ssimw_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "ssimw_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["map_and_backward_are_the_c_abi_bit_for_bit", "mean_runs_on_the_grad_out_it_is_handed_and_agrees_with_ssim",
                                   "grad_out_slice_stream_and_needs_input_grad", "memory_is_the_gradient_tensor_and_nothing_else"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
