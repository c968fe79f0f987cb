"""GPU: SSIM of float32 volumes under the three-dimensional window and its gradient (rmgr_ssim_hip_*_ssim3f*, ssim3f_kernels.hip) against
the float64 model of tests/ssim3f_model.py, and the bit patterns the header promises.  Sizes are W x H x D; arrays are (D, H, W).

Bounds.  Measured, not estimated: ssim3f_model.EMU_* hold what an fp32 emulation of the kernels' arithmetic leaves against the float64
model on the golden volumes (tests/test_ssim3f_cpu.py pins them); everything here asserts twice those figures -- per voxel, global, the
gradient error over the volume's largest float64 gradient magnitude, and max|grad| * W * H * D * R on identical volumes.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ssim3f_model as S
import ssim_amd
from conftest import ROOT

pytestmark = pytest.mark.gpu

PX_TOL, G_TOL, GRAD_TOL, IDENT_TOL = S.tolerances()
SENT = np.float32(-777.0)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def same(x, y):
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


def random_pair(size, seed, r=1.0):
    w, h, d = size
    rng = np.random.default_rng(seed)
    a = rng.random((d, h, w), dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal((d, h, w)).astype(np.float32), 0, 1).astype(np.float32)
    return a * np.float32(r), b * np.float32(r)


# ---- layouts: the same voxels stored another way ------------------------------------------------------------------------------------------
# layout(shape) -> (shape of the buffer, function that takes an array of that shape to its (D, H, W) view)
LAYOUTS = {
    "dense": lambda s: (s, lambda t: t),
    "negative step": lambda s: (s, lambda t: t[:, :, ::-1]),
    "negative stride": lambda s: (s, lambda t: t[:, ::-1, :]),
    "negative sliceStride": lambda s: (s, lambda t: t[::-1, :, :]),
    "step 2": lambda s: (s + (2,), lambda t: t[..., 1]),
    "stored (H, W, D)": lambda s: ((s[1], s[2], s[0]), lambda t: t.transpose(2, 0, 1)),
}


class Vol(object):
    """One volume in device memory under a layout: `v` (D, H, W) for an input, None for an output (every float of the buffer a sentinel)."""

    def __init__(self, ctx, shape, layout="dense", v=None):
        self.shape = tuple(shape)
        bshape, self.view = LAYOUTS[layout](self.shape)
        host = np.full(bshape, SENT, np.float32)
        if v is not None:
            self.view(host)[...] = v
        view = self.view(host)
        self.buf = ctx.upload(host)
        self.bshape = bshape
        self.ptr = self.buf.ptr + (view.ctypes.data - host.ctypes.data)
        self.strides = (view.strides[2] // 4, view.strides[1] // 4, view.strides[0] // 4)       # step, stride, sliceStride

    def result(self):
        """The output volume; every voxel written, every float outside it untouched."""
        got = self.buf.download(np.float32, self.bshape)
        out = self.view(got).copy()
        assert not np.any(bits(out) == bits(np.full(1, SENT))), "an output voxel was not written"
        self.view(got)[...] = SENT
        assert np.all(got == SENT), "a float outside the output volume was written"
        return out

    def free(self):
        self.buf.free()


def run(ctx, pairs, r, g_out=None, want=(True, True), maps=True, lin="dense", lout="dense", inputs=None):
    """Forward (sums, maps) and -- g_out given -- backward of `pairs` in ONE enqueue each, device-resident.  Returns (sums as float64,
    [map], [(dA or None, dB or None)]).  inputs: (Vol of A, Vol of B) per pair, uploaded by the caller, instead of pairs."""
    n = len(pairs) if inputs is None else len(inputs)
    own = inputs is None
    if own:
        inputs = [(Vol(ctx, a.shape, lin, a), Vol(ctx, b.shape, lin, b)) for a, b in pairs]
    d, h, w = inputs[0][0].shape
    ps = (ssim_amd.Params3F * n)()
    mvols = [Vol(ctx, (d, h, w), lout) for _ in range(n)] if maps else []
    for i, (va, vb) in enumerate(inputs):
        ps[i] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides, mvols[i].ptr if maps else None, mvols[i].strides if maps else None)
    sums = ctx.alloc(8 * n)
    ctx.enqueue_ssim3f(ps, n, r, sums.ptr)
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
        ctx.enqueue_ssim3f_grad(ps, n, r, go.ptr, arrs[0], arrs[1])
    ctx.synchronize()
    s = sums.download(np.float64, (n,))
    ms = [m.result() for m in mvols]
    grads = [(gvols[0][i].result() if want[0] else None, gvols[1][i].result() if want[1] else None) for i in range(n)] if g_out is not None else []
    for v in mvols + gvols[0] + gvols[1] + ([go] if g_out is not None else []) + [sums]:
        v.free()
    if own:
        for va, vb in inputs:
            va.free()
            vb.free()
    return s, ms, grads


def check_model(ctx, a, b, r, what, g_out=-0.75):
    """Value, map, dA alone, dB alone and both together against the float64 model at twice the emulation's figures; a gradient has the
    same bits alone and together with the other."""
    gv, gm = S.ssim(a, b, r)
    ga, gb = S.grad(a, b, r, g_out)
    vox = S.voxels(a.shape)
    s, ms, both = run(ctx, [(a, b)], r, [g_out])
    _, _, only_a = run(ctx, [(a, b)], r, [g_out], want=(True, False), maps=False)
    _, _, only_b = run(ctx, [(a, b)], r, [g_out], want=(False, True), maps=False)
    dv, dp = abs(s[0] / vox - gv), float(np.abs(ms[0].astype(np.float64) - gm).max())
    assert same(both[0][0], only_a[0][0]) and same(both[0][1], only_b[0][1]), what
    identical = np.array_equal(a, b)
    errs = []
    for got, want in ((both[0][0], ga), (both[0][1], gb)):
        assert np.all(np.isfinite(got)), what
        if identical:
            errs.append(float(np.abs(got).max()) * vox * r / abs(g_out))
        else:
            errs.append(float(np.abs(got - want).max() / np.abs(want).max()))
    print("%s: per-voxel %.3g, global %.3g, gradients %.3g %.3g%s" % (what, dp, dv, errs[0], errs[1], " (identical: max|grad| W H D R)" if identical else ""))
    assert dp <= PX_TOL and dv <= G_TOL, (what, dp, dv)
    assert max(errs) <= (IDENT_TOL if identical else GRAD_TOL), (what, errs)
    return s, ms, both


SIZES = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2),            # the axis-of-one rule on each axis
         (5, 3, 4), (4, 4, 4), (9, 9, 9),                       # axes shorter than the window, tails overlapping
         (11, 11, 11),
         (33, 33, 13),                                          # a second tile of one voxel
         (129, 17, 7),                                          # a 129th column
         (7, 9, 300), (12, 300, 3)]                             # many z-chunks, many tiles


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_model_on_every_shape_class(gpu_ctx, size):
    a, b = random_pair(size, sum(size))
    check_model(gpu_ctx, a, b, 1.0, "%dx%dx%d" % size)
    if size in ((5, 3, 4), (33, 33, 13)):
        a, b = random_pair(size, sum(size) + 1, 255.0)
        check_model(gpu_ctx, a, b, 255.0, "%dx%dx%d at range 255" % size, g_out=2.5)


@pytest.mark.parametrize("name", S.FIXTURES)
def test_model_on_the_golden_volumes(gpu_ctx, manifest, name):
    """unit, raw and scaled to range 1000; the pair of identical volumes (A against itself) in the unit form."""
    forms = S.fixture_forms(manifest, name, ("unit", "raw", "scaled"))
    assert len(forms) == 3
    for form, a, b, r in forms:
        check_model(gpu_ctx, a, b, r, "%s %s" % (name, form), g_out=1.0)
    check_model(gpu_ctx, forms[0][1], forms[0][1], 1.0, "%s against itself" % name, g_out=1.0)


def test_alone_or_anywhere_in_a_batch_and_on_a_second_call(gpu_ctx):
    size = (33, 20, 13)
    pairs = [random_pair(size, 40 + i) for i in range(3)]
    g = [-0.75, 1.5, 0.25]
    alone = [run(gpu_ctx, [pairs[i]], 1.0, [g[i]]) for i in range(3)]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        for call in range(2):                                  # a second call: the same bits
            s, ms, gr = run(gpu_ctx, [pairs[i] for i in order], 1.0, [g[i] for i in order])
            for pos, i in enumerate(order):
                assert same(s[pos:pos + 1], alone[i][0]) and same(ms[pos], alone[i][1][0]), (order, pos, call)
                assert same(gr[pos][0], alone[i][2][0][0]) and same(gr[pos][1], alone[i][2][0][1]), (order, pos, call)


@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "dense"])
def test_views_give_the_bits_of_the_dense_volume(gpu_ctx, layout):
    """Negative step, stride and sliceStride, interleaved samples (step 2) and a (D, H, W) view of data stored (H, W, D): inputs, map and
    gradients under the layout against the dense call; the sentinel gaps of the strided outputs untouched, every output voxel written
    (Vol.result)."""
    a, b = random_pair((37, 19, 14), 77)
    dense = run(gpu_ctx, [(a, b)], 1.0, [-0.75])
    for lin, lout in ((layout, "dense"), ("dense", layout), (layout, layout)):
        s, ms, gr = run(gpu_ctx, [(a, b)], 1.0, [-0.75], lin=lin, lout=lout)
        assert same(s, dense[0]) and same(ms[0], dense[1][0]), (lin, lout)
        assert same(gr[0][0], dense[2][0][0]) and same(gr[0][1], dense[2][0][1]), (lin, lout)


def test_host_entry_against_the_device_entry(gpu_ctx):
    a, b = random_pair((37, 19, 14), 78)
    s, ms, _ = run(gpu_ctx, [(a, b)], 1.0)
    want = np.float32(s[0] / S.voxels(a.shape))
    for ctx in (None, gpu_ctx):
        v, m = ssim_amd.compute_ssim3f(a, b, 1.0, want_map=True, ctx=ctx)
        assert same(np.float32([v]), np.float32([want])) and same(m, ms[0])
    # host views with negative and permuted strides are staged as they are
    ta, tb = np.ascontiguousarray(a.transpose(1, 2, 0)[::-1]), np.ascontiguousarray(b[:, :, ::-1])
    v, m = ssim_amd.compute_ssim3f(ta[::-1].transpose(2, 0, 1), tb[:, :, ::-1], 1.0, want_map=True)
    assert same(np.float32([v]), np.float32([want])) and same(m, ms[0])
    vs = ssim_amd.compute_ssim3f_batch([(a, b), (b, a), (a, a)], 1.0)
    assert same(vs[:1], np.float32([want])) and abs(float(vs[1]) - S.ssim(b, a, 1.0)[0]) <= G_TOL and abs(float(vs[2]) - 1.0) < 1e-6
    # the device entry, blocking
    va, vb = Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)
    ps = (ssim_amd.Params3F * 1)()
    ps[0] = ssim_amd.make_params3f(37, 19, 14, va.ptr, va.strides, vb.ptr, vb.strides)
    assert same(gpu_ctx.ssim3f_device(ps, 1, 1.0), np.float32([want]))
    va.free()
    vb.free()


@pytest.mark.parametrize("where", [(12, 13, 14), (0, 27, 3), (25, 0, 29)], ids=lambda p: "z%d y%d x%d" % p)
def test_the_reach_of_a_nan_voxel(gpu_ctx, where):
    """Exactly the 11^3 map voxels and the 21^3 gradient voxels around it, clipped to the volume; finite everywhere else.  The first
    position is the volume's centre voxel (the centre then is 0), the others lie on faces and edges."""
    a, b = random_pair((30, 28, 26), 5)
    a[where] = np.nan
    _, ms, gr = run(gpu_ctx, [(a, b)], 1.0, [1.0])

    def box(radius):
        m = np.zeros(a.shape, bool)
        m[tuple(slice(max(p - radius, 0), p + radius + 1) for p in where)] = True
        return m
    assert np.array_equal(np.isnan(ms[0]), box(5)) and np.all(np.isfinite(ms[0][~box(5)]))
    for g in gr[0]:
        assert np.array_equal(np.isnan(g), box(10)) and np.all(np.isfinite(g[~box(10)]))


def test_offsets_that_need_more_than_32_bits(gpu_ctx):
    """A 20 x 18 x 3 volume whose slices lie 2^30 floats (4 GiB) apart -- A, B, the map and both gradients, each at its own place in one
    device-only buffer of 8 GiB and a little: slice 1 is 2^32 bytes and slice 2 is 2^33 bytes from slice 0, so an offset truncated to 32
    bits lands on slice 0.  Also with the slices in descending order (sliceStride = -2^30).  The bits of the dense call."""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    w, h, d, far = 20, 18, 3, 1 << 30
    a, b = random_pair((w, h, d), 9)
    dense = run(ctx, [(a, b)], 1.0, [-0.75])
    room = 1024                                                   # floats per item and slice (>= w * h)
    buf = ctx.alloc(4 * (2 * far + 5 * room))

    def at(item, z):
        return buf.ptr + 4 * (z * far + item * room)

    def put(item, vol):
        for z in range(d):
            plane = np.ascontiguousarray(vol[z])
            assert lib.rmgr_ssim_hip_memcpy_h2d(ctx.handle, at(item, z), plane.ctypes.data, plane.nbytes) == 0

    def get(item):
        return np.stack([ctx.download(at(item, z), np.float32, (h, w)) for z in range(d)])
    for sign in (1, -1):
        order = a[::sign], b[::sign]                              # slice z of the volume is stored at far * z (sign 1) or far * (d - 1 - z)
        put(0, order[0])
        put(1, order[1])
        for item in (2, 3, 4):
            put(item, np.full((d, h, w), SENT, np.float32))
        z0 = 0 if sign == 1 else d - 1
        strides = (1, w, sign * far)
        ps = (ssim_amd.Params3F * 1)()
        ps[0] = ssim_amd.make_params3f(w, h, d, at(0, z0), strides, at(1, z0), strides, at(2, z0), strides)
        ga, gb = (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)()
        ga[0], gb[0] = ssim_amd.Grad3F(at(3, z0), *strides), ssim_amd.Grad3F(at(4, z0), *strides)
        sums, go = ctx.alloc(8), ctx.upload(np.float32([-0.75]))
        ctx.enqueue_ssim3f(ps, 1, 1.0, sums.ptr)
        ctx.enqueue_ssim3f_grad(ps, 1, 1.0, go.ptr, ga, gb)
        ctx.synchronize()
        assert same(sums.download(np.float64, (1,)), dense[0]), sign
        assert same(get(2)[::sign], dense[1][0]), sign
        assert same(get(3)[::sign], dense[2][0][0]) and same(get(4)[::sign], dense[2][0][1]), sign
        sums.free()
        go.free()
    buf.free()


def test_sub_batches_of_the_backward_scratch(gpu_ctx):
    """The backward keeps 16 bytes of coefficients per voxel for both gradients (include/rmgr/ssim-hip.h) in sub-batches of 1 GiB: one more
    volume of 160^3 than a sub-batch holds runs in two.  Every pair reads the same two device volumes; every gradient has the bits of the
    lone call."""
    n = (1 << 30) // (16 * 160 ** 3) + 1
    assert n == 17
    a, b = random_pair((160, 160, 160), 3)
    va, vb = Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)
    lone = run(gpu_ctx, None, 1.0, [-0.75], maps=False, inputs=[(va, vb)])
    assert np.abs(lone[2][0][0]).max() > 0 and np.abs(lone[2][0][1]).max() > 0
    s, _, gr = run(gpu_ctx, None, 1.0, [-0.75] * n, maps=False, inputs=[(va, vb)] * n)
    for i in range(n):
        assert same(s[i:i + 1], lone[0]) and same(gr[i][0], lone[2][0][0]) and same(gr[i][1], lone[2][0][1]), i
    va.free()
    vb.free()


def test_one_context_shared_with_the_2d_paths(gpu_ctx):
    """ssim3f forward and backward interleaved with ssimf and msssimf calls on one context without a host wait: every byte is that of the
    call issued alone (the descriptor ring, the cell partials and the scratch are shared in stream order)."""
    ctx = gpu_ctx
    a, b = random_pair((40, 36, 20), 21)
    va, vb = Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b)
    d, h, w = a.shape
    rng = np.random.default_rng(22)
    pa, pb = rng.random((256, 272), dtype=np.float32), rng.random((256, 272), dtype=np.float32)
    da, db = ctx.upload(pa), ctx.upload(pb)
    p2 = (ssim_amd.ParamsF * 1)()
    p2[0] = ssim_amd.make_params_f(272, 256, da.ptr, 1, 272, db.ptr, 1, 272)
    go = ctx.upload(np.float32([-0.75]))

    def issue(wait):
        outs = {"s3": ctx.alloc(8), "m3": ctx.alloc(4 * a.size), "ga": ctx.alloc(4 * a.size), "gb": ctx.alloc(4 * a.size), "s2": ctx.alloc(8),
                "g2": ctx.alloc(4 * pa.size), "ms": ctx.alloc(8), "means": ctx.alloc(8 * 10), "s3b": ctx.alloc(8)}
        p3 = (ssim_amd.Params3F * 1)()
        p3[0] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides, outs["m3"].ptr)
        ga, gb, g2 = (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)(), (ssim_amd.GradF * 1)()
        ga[0], gb[0], g2[0] = ssim_amd.Grad3F(outs["ga"].ptr, 1, w, w * h), ssim_amd.Grad3F(outs["gb"].ptr, 1, w, w * h), ssim_amd.GradF(outs["g2"].ptr, 1, 272)
        steps = [lambda: ctx.enqueue_ssim3f(p3, 1, 1.0, outs["s3"].ptr),
                 lambda: ctx.enqueue_ssimf(p2, 1, 1.0, outs["s2"].ptr),
                 lambda: ctx.enqueue_ssim3f_grad(p3, 1, 1.0, go.ptr, ga, gb),
                 lambda: ctx.enqueue_msssimf(p2, 1, 1.0, outs["ms"].ptr, outs["means"].ptr),
                 lambda: ctx.enqueue_ssimf_grad(p2, 1, 1.0, go.ptr, g2, None),
                 lambda: ctx.enqueue_ssim3f(p3, 1, 1.0, outs["s3b"].ptr)]
        for step in steps:
            step()
            if wait:
                ctx.synchronize()
        ctx.synchronize()
        got = {k: v.download(np.uint8, (v.nbytes,)) for k, v in outs.items()}
        for v in outs.values():
            v.free()
        return got
    alone, mixed = issue(True), issue(False)
    for k in alone:
        assert np.array_equal(alone[k], mixed[k]), k
    assert np.array_equal(alone["s3"], alone["s3b"])
    gv, _ = S.ssim(a, b, 1.0)
    assert abs(float(alone["s3"].view(np.float64)[0]) / S.voxels(a.shape) - gv) <= G_TOL
    for v in (va, vb, da, db, go):
        v.free()


def test_many_volumes_in_one_launch(gpu_ctx):
    """300 volumes of 9 x 9 x 40 in one enqueue: value, map and both gradients of every one have the bits they have alone."""
    ctx, n, size = gpu_ctx, 300, (9, 9, 40)
    w, h, d = size
    rng = np.random.default_rng(8)
    a = rng.random((n, d, h, w), dtype=np.float32)
    b = np.clip(a + np.float32(0.1) * rng.standard_normal(a.shape).astype(np.float32), 0, 1).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    vox = w * h * d
    da, db, go = ctx.upload(a), ctx.upload(b), ctx.upload(g)

    def issue(groups):
        m, ga, gb, s = ctx.alloc(4 * a.size), ctx.alloc(4 * a.size), ctx.alloc(4 * a.size), ctx.alloc(8 * n)
        for first, count in groups:
            ps, pa, pb = (ssim_amd.Params3F * count)(), (ssim_amd.Grad3F * count)(), (ssim_amd.Grad3F * count)()
            for j in range(count):
                off = 4 * vox * (first + j)
                ps[j] = ssim_amd.make_params3f(w, h, d, da.ptr + off, (1, w, w * h), db.ptr + off, (1, w, w * h), m.ptr + off)
                pa[j], pb[j] = ssim_amd.Grad3F(ga.ptr + off, 1, w, w * h), ssim_amd.Grad3F(gb.ptr + off, 1, w, w * h)
            ctx.enqueue_ssim3f(ps, count, 1.0, s.ptr + 8 * first)
            ctx.enqueue_ssim3f_grad(ps, count, 1.0, go.ptr + 4 * first, pa, pb)
        ctx.synchronize()
        got = [s.download(np.float64, (n,))] + [v.download(np.float32, a.shape) for v in (m, ga, gb)]
        for v in (m, ga, gb, s):
            v.free()
        return got
    together, alone = issue([(0, n)]), issue([(i, 1) for i in range(n)])
    for x, y in zip(together, alone):
        assert same(x, y)
    for i in (0, 137, 299):
        gv, gm = S.ssim(a[i], b[i], 1.0)
        assert abs(together[0][i] / vox - gv) <= G_TOL and np.abs(together[1][i] - gm).max() <= PX_TOL
        want = S.grad(a[i], b[i], 1.0, float(g[i]))
        for got, wnt in ((together[2][i], want[0]), (together[3][i], want[1])):
            assert np.abs(got - wnt).max() / np.abs(wnt).max() <= GRAD_TOL
    for v in (da, db, go):
        v.free()


# ---- PyTorch -----------------------------------------------------------------------------------------------------------------------------
# torch brings its own HIP runtime; the checks run in ONE child process (tests/tools/ssim3f_torch_checks.py) that imports torch before the
# library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "ssim3f_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "ssim3f_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["value_and_gradients_against_the_model", "loss_forms", "non_contiguous_and_expanded_inputs", "side_stream",
                                   "empty_leading_shape", "ssim_on_the_same_5d_tensor_is_unchanged_and_differs"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
