"""GPU: SSIM of float16 / bfloat16 volumes, its gradient and the gradient of its map (rmgr_ssim_hip_*_ssim3h*, ssim3h_kernels.hip) against
the float32 entries, BIT FOR BIT.  Sizes are W x H x D; arrays are (D, H, W); 16-bit samples travel as uint16 bit patterns.

The contract (include/rmgr/ssim-hip.h): value, map and fp64 sums have the bits rmgr_ssim_hip_enqueue_ssim3f gives on the widened volumes;
a gradient voxel is the float32 value of _enqueue_ssim3f_grad / _ssim3f_map_grad rounded once, to nearest-even, into the inputs'
encoding.  So every comparison here runs the float32 entry in the same test on halfmodel.widen(samples) and compares bits -- gradients
against halfmodel.round_to(float32 gradient) -- and no tolerance is new.  NaN is compared as NaN (halfmodel.same / same_f32), which only
matters where the float32 path itself yields NaN.  The one comparison with a bound is the golden-derived volumes as stored against the
float64 model at ssim3f_model.tolerances(); tests/test_ssim3h_cpu.py checks its input condition.

Shapes, the smallest at which a tile, cell, chunk or window edge can go wrong: 1x1x1; 3x5x2; 5x3x40 (both lateral axes shorter than the
window); 17x17x9 (one voxel past a 16-voxel tile on both axes and past an 8-slice cell); 33x20x13; and 17x17x131 inside a launch of
enough volumes that tests/ssim3f_plan.py, at the device's CU count, gives chunks of at least 16 slices (asserted, never skipped).

All outputs of a call -- maps, gradient volumes -- live in ONE buffer each with sentinel gaps (Arena); after every call the gaps and every
element of a strided output's buffer outside the volume are asserted untouched.

After a return code that is neither success nor EINVAL the module starts nothing more on the GPU (test_gpu_ssimk's _device_error, shared
with that module).  Every test frees its buffers.  The module prints its wall time and its peak device memory when it ends.

Cost, measured on an MI355X: the 76 tests take 7.3 s together, nearly all of it the start of the PyTorch child process; no other test
takes more than 0.05 s; the device holds 64 MiB more than before the module at the peak (the 65537-volume call).
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

import halfmodel as HM
import ssim3f_model as S
import ssim3f_plan as P
import ssim3h_inputs as IN
import ssim_amd
from conftest import ROOT
from test_gpu_ssim3f import LAYOUTS as LAYOUTS3F
from test_gpu_ssimk import _device_error

pytestmark = pytest.mark.gpu

ENC = pytest.mark.parametrize("enc", HM.ENCODINGS)
SHAPES = [(1, 1, 1), (3, 5, 2), (5, 3, 40), (17, 17, 9), (33, 20, 13)]
BY_SHAPE = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
GAP = 32                                                   # sentinel elements around every volume of an arena
SENT = {np.dtype(np.float32): np.float32(-777.0), np.dtype(np.uint16): np.uint16(0x7BCD), np.dtype(np.float64): np.float64(-777.0)}
NAN16 = {HM.F16: 0x7E00, HM.BF16: 0x7FC0}
MAX16 = {HM.F16: 65504.0, HM.BF16: 3.3895313892515355e38}

LAYOUTS = dict(LAYOUTS3F)
LAYOUTS["odd offset"] = lambda s: ((s[0] * s[1] * s[2] + 1,), lambda t: t[1:].reshape(s))       # the base one sample past a 4-byte boundary
LAYOUTS["stored (W, D, H)"] = lambda s: ((s[2], s[0], s[1]), lambda t: t.transpose(1, 2, 0))


def call(fn, *args):
    """One library call.  Any failure ends the test (SsimError); one that is neither success nor EINVAL is a device error, after which
    this module starts nothing more on the GPU."""
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    try:
        return fn(*args)
    except ssim_amd.SsimError as e:
        if e.errno != 22:
            _device_error.append(e.errno)
        raise


class Device(object):
    def __init__(self, ctx):
        self.ctx, self.t0 = ctx, time.time()
        said = re.search(r"(\d+) CUs", ctx.describe())
        assert said, ctx.describe()
        self.cus = int(said.group(1))
        self.free0 = self.min_free = ssim_amd.memory_info(ctx)[0]

    def sample(self):
        self.min_free = min(self.min_free, ssim_amd.memory_info(self.ctx)[0])

    def close(self):
        self.ctx.trim()
        print("\n16-bit volumes: %d CUs; module wall time %.1f s; peak device memory in use by the module %.1f MiB" % (
            self.cus, time.time() - self.t0, (self.free0 - self.min_free) / 2.0 ** 20))


@pytest.fixture(scope="module")
def device(gpu_ctx):
    d = Device(gpu_ctx)
    yield d
    d.close()


class Arena(object):
    """Volumes of one element type in ONE device buffer, each under a layout of its own, GAP sentinel elements before, between and after
    them.  add() before upload(); at() and results() after."""

    def __init__(self, dtype):
        self.dtype, self.items, self.n, self.buf = np.dtype(dtype), [], GAP, None

    def add(self, shape, layout="dense", v=None):
        bshape, view = LAYOUTS[layout](tuple(shape))
        self.items.append((self.n, bshape, view, v))
        self.n += int(np.prod(bshape)) + GAP
        return len(self.items) - 1

    def _view(self, host, i):
        off, bshape, view, _ = self.items[i]
        return view(host[off:off + int(np.prod(bshape))].reshape(bshape))

    def upload(self, ctx):
        assert not _device_error, "an earlier call left a device error: %r" % _device_error
        self.host = np.full(self.n, SENT[self.dtype], self.dtype)
        for i, it in enumerate(self.items):
            if it[3] is not None:
                self._view(self.host, i)[...] = it[3]
        self.buf = ctx.upload(self.host)
        return self

    def at(self, i):
        """(device pointer of voxel (0, 0, 0), (step, stride, sliceStride) in elements)."""
        v = self._view(self.host, i)
        es = self.dtype.itemsize
        return self.buf.ptr + (v.ctypes.data - self.host.ctypes.data), (v.strides[2] // es, v.strides[1] // es, v.strides[0] // es)

    def results(self, written=False):
        """Every output volume; every element outside them untouched.  written: no output element still holds the sentinel."""
        got = self.buf.download(self.dtype, (self.n,))
        outs = []
        for i in range(len(self.items)):
            v = self._view(got, i)
            outs.append(v.copy())
            if written:
                assert not np.any(outs[-1] == SENT[self.dtype]), "an output voxel was not written"
            v[...] = SENT[self.dtype]
        assert np.all(got == SENT[self.dtype]), "an element outside the output volumes was written"
        return outs

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None


def run(device, enc, pairs, r, g_out=None, gmaps=None, want=(True, True), maps=True, lin="dense", lout="dense", lmap=None, lg="dense",
        zero_slice=False):
    """Forward (sums, maps) and backward of `pairs` in ONE enqueue each, device-resident.  enc None: the float32 entries on float32
    volumes; else the ssim3h entries on uint16 bit patterns.  g_out: one dLoss/dS per pair (the _grad entry); gmaps: one float32 volume
    per pair, or one float per pair with the strides (0, 0, 0) (a scalar), under the layout lg (the _map_grad entry).  maps: True (every
    pair gets a map, under the layout lmap or lout), False, or {volume: layout} for the volumes that get one.  zero_slice: a depth;
    the inputs are one slice each, addressed with sliceStride 0 as a volume of that depth.  Returns
    (sums as float64, [map], [(dA or None, dB or None)])."""
    ctx, n = device.ctx, len(pairs)
    half = enc is not None
    dt = np.uint16 if half else np.float32
    PS, GR = (ssim_amd.Params3H, ssim_amd.Grad3H) if half else (ssim_amd.Params3F, ssim_amd.Grad3F)
    make = ssim_amd.make_params3h if half else ssim_amd.make_params3f
    d, h, w = pairs[0][0].shape
    if zero_slice:
        d = zero_slice
    arenas = []
    try:
        ins = Arena(dt)
        for a, b in pairs:
            ins.add(a.shape, lin, a)
            ins.add(b.shape, lin, b)
        arenas.append(ins.upload(ctx))
        mar = Arena(np.float32)
        map_at = dict(maps) if isinstance(maps, dict) else dict((i, lmap or lout) for i in range(n)) if maps else {}
        map_idx = dict((i, mar.add((d, h, w), map_at[i])) for i in sorted(map_at))
        arenas.append(mar.upload(ctx))
        sums = Arena(np.float64)
        sums.add((1, 1, n))
        arenas.append(sums.upload(ctx))
        ps = (PS * n)()
        for i in range(n):
            (pa, sa), (pb, sb) = ins.at(2 * i), ins.at(2 * i + 1)
            if zero_slice:
                sa, sb = sa[:2] + (0,), sb[:2] + (0,)
            mp, ms = mar.at(map_idx[i]) if i in map_idx else (None, None)
            ps[i] = make(w, h, d, pa, sa, pb, sb, mp, ms)
        if half:
            call(ctx.enqueue_ssim3h, ps, n, r, enc, sums.at(0)[0])
        else:
            call(ctx.enqueue_ssim3f, ps, n, r, sums.at(0)[0])
        backward = g_out is not None or gmaps is not None
        gar = Arena(dt)
        if backward:
            arrs, idx = [None, None], [[], []]
            for k in range(2):
                if want[k]:
                    for i in range(n):
                        idx[k].append(gar.add((d, h, w), lout))
            arenas.append(gar.upload(ctx))
            for k in range(2):
                if want[k]:
                    arrs[k] = (GR * n)()
                    for i in range(n):
                        p, s = gar.at(idx[k][i])
                        arrs[k][i] = GR(p, *s)
            up = Arena(np.float32)
            if g_out is not None:
                up.add((1, 1, n), "dense", np.asarray(g_out, np.float32).reshape(1, 1, n))
                arenas.append(up.upload(ctx))
                if half:
                    call(ctx.enqueue_ssim3h_grad, ps, n, r, enc, up.at(0)[0], arrs[0], arrs[1])
                else:
                    call(ctx.enqueue_ssim3f_grad, ps, n, r, up.at(0)[0], arrs[0], arrs[1])
            else:
                gm = (ssim_amd.GradOut3F * n)()
                for i, k in enumerate(gmaps):
                    k = np.asarray(k, np.float32)
                    up.add((1, 1, 1) if k.ndim == 0 else k.shape, "dense" if k.ndim == 0 else lg, k)
                arenas.append(up.upload(ctx))
                for i, k in enumerate(gmaps):
                    p, s = up.at(i)
                    gm[i] = ssim_amd.GradOut3F(p, *((0, 0, 0) if np.ndim(k) == 0 else s))
                if half:
                    call(ctx.enqueue_ssim3h_map_grad, ps, n, r, enc, gm, arrs[0], arrs[1])
                else:
                    call(ctx.enqueue_ssim3f_map_grad, ps, n, r, gm, arrs[0], arrs[1])
        call(ctx.synchronize)
        device.sample()
        s = sums.results()[0].reshape(n)
        ms = mar.results(written=True)                     # in ascending order of the volumes that have a map
        grads = []
        if backward:
            got = gar.results()
            grads = [(got[idx[0][i]] if want[0] else None, got[idx[1][i]] if want[1] else None) for i in range(n)]
            up.results()
        ins.results()                                      # the inputs and everything around them are unchanged
        return s, ms, grads
    finally:
        for a in arenas:
            a.free()


def widened(pairs, enc):
    return [(HM.widen(a, enc), HM.widen(b, enc)) for a, b in pairs]


def same64(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


def check_against_float32(device, enc, pairs, r, what, **kw):
    """One call of the 16-bit entries against the same call of the float32 entries on the widened volumes: sums and maps bit for bit,
    gradients against the float32 gradients rounded once.  Returns the 16-bit results."""
    got = run(device, enc, pairs, r, **kw)
    ref = run(device, None, widened(pairs, enc), r, **kw)
    assert same64(got[0], ref[0]), (what, got[0], ref[0])
    for m, wm in zip(got[1], ref[1]):
        assert HM.same_f32(m, wm), what
    assert len(got[2]) == len(ref[2])
    for (ga, gb), (fa, fb) in zip(got[2], ref[2]):
        for g, f in ((ga, fa), (gb, fb)):
            assert (g is None) == (f is None), what
            if g is not None:
                assert g.dtype == np.uint16 and HM.same(g, HM.round_to(f, enc), enc), what
    return got, ref


def normal_scale(device, enc, pair, r):
    """A dLoss/dS that puts the float16 gradients of this pair in the normal range: the largest float32 gradient magnitude becomes 1."""
    _, _, gr = run(device, None, widened([pair], enc), r, g_out=[1.0], maps=False)
    top = max(float(np.nanmax(np.abs(g))) for g in gr[0])
    return 1.0 / top if top > 0 else 1.0


# ---- forward -------------------------------------------------------------------------------------------------------------------------

def check_value_entries(device, enc, pair, fp64_sum, dense_map):
    """The value of one pair through the blocking entries -- the float32 host entry on the widened volumes, the 16-bit host entry (on the
    module's context, on a default context and in a batch) and the 16-bit device entry -- against the enqueue entry's fp64 sum and map."""
    d, h, w = pair[0].shape
    want = np.float32(fp64_sum / S.voxels((d, h, w)))
    wa, wb = widened([pair], enc)[0]
    fv, fm = call(ssim_amd.compute_ssim3f, wa, wb, 1.0, True, device.ctx)
    assert np.float32(fv).tobytes() == want.tobytes() and HM.same_f32(fm, dense_map)
    # the host entry: float16 arrays as they are, bfloat16 as uint16 bit patterns
    (ha, st), (hb, _) = HM.host_array(pair[0], enc), HM.host_array(pair[1], enc)
    for ctx in (device.ctx, None):
        v, m = call(ssim_amd.compute_ssim3h, ha, hb, 1.0, st, True, ctx)
        assert np.float32(v).tobytes() == want.tobytes() and HM.same_f32(m, dense_map), (pair[0].shape, ctx)
    vs = call(ssim_amd.compute_ssim3h_batch, [(ha, hb), (hb, ha)], 1.0, st, device.ctx)
    assert vs[:1].tobytes() == want.tobytes()
    # the blocking device entry
    ins = Arena(np.uint16)
    ins.add(pair[0].shape, "dense", pair[0])
    ins.add(pair[1].shape, "dense", pair[1])
    ins.upload(device.ctx)
    try:
        ps = (ssim_amd.Params3H * 1)()
        ps[0] = ssim_amd.make_params3h(w, h, d, ins.at(0)[0], ins.at(0)[1], ins.at(1)[0], ins.at(1)[1])
        assert call(device.ctx.ssim3h_device, ps, 1, 1.0, enc).tobytes() == want.tobytes()
    finally:
        ins.free()


@ENC
@BY_SHAPE
def test_forward_has_the_bits_of_the_float32_path(device, enc, shape):
    """Value (blocking device and host entries), fp64 sums (the enqueue entry) and the map in dense, step-2 and negative-sliceStride
    layouts over a sentinel prefill."""
    pair = IN.random_pair(shape, sum(shape), enc)
    for lmap in ("dense", "step 2", "negative sliceStride"):
        (s, ms, _), _ = check_against_float32(device, enc, [pair], 1.0, ("forward", shape, lmap), lmap=lmap)
    check_value_entries(device, enc, pair, s[0], ms[0])


def test_host_entry_stages_views_as_they_are(device):
    """Host views with negative, permuted and interleaved strides, a float32 map at strides of its own: staged 2 bytes per sample."""
    a, b = IN.random_pair((21, 18, 7), 3, HM.F16)
    v0, m0 = call(ssim_amd.compute_ssim3h, a.view(np.float16), b.view(np.float16), 1.0, None, True, device.ctx)
    ta = np.ascontiguousarray(a.transpose(1, 2, 0)[::-1])                      # stored (H, W, D), rows reversed
    tb = np.zeros(b.shape + (2,), np.uint16)
    tb[..., 1] = b[:, :, ::-1]
    v, m = call(ssim_amd.compute_ssim3h, ta[::-1].transpose(2, 0, 1).view(np.float16), tb[..., 1][:, :, ::-1].view(np.float16), 1.0, None, True, device.ctx)
    assert np.float32(v).tobytes() == np.float32(v0).tobytes() and HM.same_f32(m, m0)
    # a strided map through the C entry
    big = np.full((7, 18, 42), -777.0, np.float32)
    ps = (ssim_amd.Params3H * 1)()
    ps[0] = ssim_amd.make_params3h(21, 18, 7, a.ctypes.data, (1, 21, 21 * 18), b.ctypes.data, (1, 21, 21 * 18),
                                   big[::-1, :, 1::2].ctypes.data, (2, 42, -42 * 18))
    out = (ctypes.c_float * 1)()
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    rc = device.ctx.lib.rmgr_ssim_hip_compute_ssim3h_host(device.ctx.handle, 1, ps, ssim_amd.SAMPLE_F16, 1.0, out)
    if rc not in (0, 22):
        _device_error.append(rc)
    assert rc == 0, rc
    assert HM.same_f32(big[::-1, :, 1::2], m0) and np.all(big[:, :, 0::2] == -777.0)


# ---- gradient and map gradient -------------------------------------------------------------------------------------------------------

@ENC
@BY_SHAPE
def test_gradients_are_the_float32_gradients_rounded_once(device, enc, shape):
    """dA alone, dB alone and both, with gOut scaled so that float16 gradients are normal numbers; each gradient has the same bits alone
    and together with the other; the map gradient with the constant gMap float(gOut / (W H D)) -- as a volume and as one float with
    strides (0, 0, 0) -- has the bits of the _grad entry."""
    pair = IN.random_pair(shape, 100 + sum(shape), enc)
    g = -0.75 * normal_scale(device, enc, pair, 1.0)
    (_, _, both), (_, _, f32) = check_against_float32(device, enc, [pair], 1.0, ("both", shape), g_out=[g], maps=False)
    (_, _, only_a), _ = check_against_float32(device, enc, [pair], 1.0, ("dA", shape), g_out=[g], want=(True, False), maps=False)
    (_, _, only_b), _ = check_against_float32(device, enc, [pair], 1.0, ("dB", shape), g_out=[g], want=(False, True), maps=False)
    assert np.array_equal(both[0][0], only_a[0][0]) and np.array_equal(both[0][1], only_b[0][1]) and only_a[0][1] is None and only_b[0][0] is None
    top = max(float(np.abs(f).max()) for f in f32[0])
    assert 0.7 < top < 0.8 or shape == (1, 1, 1), top                          # the scale did what it is for
    if enc == HM.F16 and shape != (1, 1, 1):
        assert not np.all(HM.is_subnormal(both[0][0], enc) | (both[0][0] & 0x7FFF == 0))
    k = np.float32(float(np.float32(g)) / S.voxels(pair[0].shape))
    for gm in (np.full(pair[0].shape, k, np.float32), k):
        for want in ((True, True), (True, False), (False, True)):
            _, _, ident = run(device, enc, [pair], 1.0, gmaps=[gm], want=want, maps=False)
            for side in range(2):
                assert (ident[0][side] is None) == (not want[side])
                if want[side]:
                    assert np.array_equal(ident[0][side], both[0][side]), (shape, want, side, np.ndim(gm))


@ENC
def test_subnormal_results_are_kept_and_overflow_gives_inf(device, enc):
    """Unscaled, the gradient of a mean SSIM is of order 1 / (W H D): among float16 subnormals, which are kept, not flushed.  Scaled far
    up, some voxels overflow to Inf.  Both through the _grad and the _map_grad entry (bfloat16 has the exponent range of float32: there
    the unscaled results are normal numbers, and the overflow is reached through gMap, which is not divided by W H D)."""
    pair = IN.random_pair((33, 20, 13), 7, enc)
    (_, _, gr), (_, _, f32) = check_against_float32(device, enc, [pair], 1.0, "unscaled", g_out=[1.0], maps=False)
    if enc == HM.F16:
        for g in gr[0]:
            sub = HM.is_subnormal(g, enc)
            assert sub.sum() > g.size // 4, int(sub.sum())                          # about a third of the voxels lie below 6.1e-5
    else:
        assert not np.any(HM.is_subnormal(gr[0][0], enc))
    vox = S.voxels(pair[0].shape)
    top = max(float(np.abs(f).max()) for f in f32[0]) * vox                    # the largest |gradient| per unit of k
    k = np.float32(4.0 * MAX16[enc] / top)                                     # about a quarter of the voxels lie above a quarter of the largest
    (_, _, gr), _ = check_against_float32(device, enc, [pair], 1.0, "overflow through gMap", gmaps=[k], maps=False)
    for g in gr[0]:
        inf = (g & 0x7FFF) == (0x7C00 if enc == HM.F16 else 0x7F80)
        print("%s: %d of %d voxels overflow to Inf at k = %g" % (enc, int(inf.sum()), g.size, float(k)))
        assert 0 < inf.sum() < g.size
    if enc == HM.F16:
        (_, _, gr2), _ = check_against_float32(device, enc, [pair], 1.0, "overflow through gOut", g_out=[float(k) * vox], maps=False)
        assert any(np.any((g & 0x7FFF) == 0x7C00) for g in gr2[0])


@ENC
@pytest.mark.parametrize("lg", ["dense", "negative sliceStride", "negative step", "stored (H, W, D)", "step 2"])
def test_map_gradient_for_a_per_voxel_upstream_gradient(device, enc, lg):
    """A random signed gMap under a mask, stored densely, with negative strides, permuted and interleaved: the float32 map gradient
    rounded once; every view the bits of the dense gMap."""
    shape = (33, 20, 13)
    pair = IN.random_pair(shape, 11, enc)
    rng = np.random.default_rng(12)
    gm = (rng.standard_normal(pair[0].shape) * (rng.random(pair[0].shape) < 0.6)).astype(np.float32)
    for want in ((True, True), (True, False), (False, True)):
        check_against_float32(device, enc, [pair], 1.0, ("map grad", lg, want), gmaps=[gm], want=want, maps=False, lg=lg)


# ---- views of the samples ------------------------------------------------------------------------------------------------------------

@ENC
@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "dense"])
def test_views_give_the_bits_of_the_dense_volume(device, enc, layout):
    """An odd sample offset (2-byte but not 4-byte aligned base), interleaved samples, negative and permuted strides: inputs, and
    gradient volumes, under the layout against the dense call and against the float32 path."""
    if layout == "odd offset":
        ar = Arena(np.uint16)
        ar.add((2, 2, 2), layout)
        ar.upload(device.ctx)
        try:
            assert ar.at(0)[0] % 4 == 2
        finally:
            ar.free()
    pair = IN.random_pair((37, 19, 14), 77, enc)
    g = 0.5 * normal_scale(device, enc, pair, 1.0)
    dense, _ = check_against_float32(device, enc, [pair], 1.0, "dense", g_out=[g])
    for lin, lout in ((layout, "dense"), ("dense", layout), (layout, layout)):
        s, ms, gr = run(device, enc, [pair], 1.0, g_out=[g], lin=lin, lout=lout, lmap="dense")
        assert same64(s, dense[0]) and HM.same_f32(ms[0], dense[1][0]), (lin, lout)
        assert np.array_equal(gr[0][0], dense[2][0][0]) and np.array_equal(gr[0][1], dense[2][0][1]), (lin, lout)


@ENC
def test_a_zero_stride_is_an_expanded_axis(device, enc):
    """One slice addressed with sliceStride 0 as a volume of 9 slices: the bits of the 9 copies stored densely."""
    a, b = IN.random_pair((17, 17, 1), 5, enc)
    full = (np.repeat(a, 9, axis=0), np.repeat(b, 9, axis=0))
    g = 0.5 * normal_scale(device, enc, full, 1.0)
    dense, _ = check_against_float32(device, enc, [full], 1.0, "dense", g_out=[g])
    s, ms, gr = run(device, enc, [(a, b)], 1.0, g_out=[g], zero_slice=9)
    assert same64(s, dense[0]) and HM.same_f32(ms[0], dense[1][0])
    assert np.array_equal(gr[0][0], dense[2][0][0]) and np.array_equal(gr[0][1], dense[2][0][1])


# ---- special values ------------------------------------------------------------------------------------------------------------------

def _box(shape, where, radius):
    m = np.zeros(shape, bool)
    m[tuple(slice(max(p - radius, 0), p + radius + 1) for p in where)] = True
    return m


@ENC
@pytest.mark.parametrize("where", [(12, 13, 14), (0, 27, 3)], ids=lambda p: "z%d y%d x%d" % p)
def test_the_reach_of_a_nan(device, enc, where):
    """A NaN sample: exactly the 11^3 map voxels and the 21^3 gradient voxels around it, clipped; a NaN in gMap: 11^3.  The first
    position is the volume's centre voxel: the centre then is 0 (the float32 path decides the same; every finite bit is compared).
    bfloat16: a NaN stays a NaN after narrowing."""
    a, b = IN.random_pair((30, 28, 26), 5, enc)
    an = a.copy()
    an[where] = NAN16[enc]
    (_, ms, gr), _ = check_against_float32(device, enc, [(an, b)], 1.0, "NaN sample", g_out=[1000.0])
    assert np.array_equal(np.isnan(ms[0]), _box(a.shape, where, 5)) and np.all(np.isfinite(ms[0][~_box(a.shape, where, 5)]))
    for g in gr[0]:
        assert np.array_equal(HM.is_nan(g, enc), _box(a.shape, where, 10))
        assert np.all(np.isfinite(HM.widen(g, enc)[~_box(a.shape, where, 10)]))
    gm = np.full(a.shape, 0.01, np.float32)
    gm[where] = np.nan
    (_, _, gr), _ = check_against_float32(device, enc, [(a, b)], 1.0, "NaN in gMap", gmaps=[gm], maps=False)
    for g in gr[0]:
        assert np.array_equal(HM.is_nan(g, enc), _box(a.shape, where, 5))
        assert np.all(np.isfinite(HM.widen(g, enc)[~_box(a.shape, where, 5)]))


@ENC
def test_subnormal_samples_and_samples_above_the_data_range(device, enc):
    """A volume of subnormals of the encoding (float16: bit patterns 1 .. 1023, at a data range of their size; bfloat16: 1 .. 127, which
    are subnormals of float32 as well, at range 1: the bits decide); samples above dataRange are used as stored, and a centre sample above
    it makes the centre 0."""
    rng = np.random.default_rng(9)
    shape = (9, 17, 17)
    top = 1023 if enc == HM.F16 else 127
    a = rng.integers(1, top + 1, shape).astype(np.uint16)
    b = np.clip(a.astype(np.int32) + rng.integers(-40, 41, shape), 1, top).astype(np.uint16)
    assert np.all(HM.is_subnormal(a, enc)) and np.all(HM.is_subnormal(b, enc))
    r = float(HM.widen(np.uint16([1023]), HM.F16)[0]) if enc == HM.F16 else 1.0
    (s, ms, _), _ = check_against_float32(device, enc, [(a, b)], r, "subnormals", g_out=[1.0])
    if enc == HM.F16:
        assert 0.0 < s[0] / S.voxels(shape) < 0.999                            # the samples were not flushed to zero: the pair differs
    # samples above the data range, the centre among them
    a, b = IN.random_pair((17, 17, 9), 10, enc, r=4.0)
    a[4, 8, 8], b[4, 8, 8] = HM.round_to(np.float32([3.5, -2.25]), enc)           # both centre samples chosen: magnitudes above the range
    assert HM.widen(a, enc)[4, 8, 8] == 3.5 and HM.widen(b, enc)[4, 8, 8] == -2.25 and (HM.widen(a, enc) > 1.0).sum() > a.size // 2
    g = normal_scale(device, enc, (a, b), 1.0)
    (s, _, _), _ = check_against_float32(device, enc, [(a, b)], 1.0, "above the data range", g_out=[g])
    gv, _ = S.ssim(*widened([(a, b)], enc)[0], 1.0)
    assert abs(s[0] / S.voxels(a.shape) - gv) <= 1e-3                          # used as stored, not clipped (a coarse sanity bound; the bits above are the check)


# ---- scheduling ----------------------------------------------------------------------------------------------------------------------

@ENC
def test_alone_or_anywhere_in_a_batch_and_on_a_second_call(device, enc):
    size = (33, 20, 13)
    pairs = [IN.random_pair(size, 40 + i, enc) for i in range(3)]
    g = [-0.75e4, 1.5e4, 0.25e4]
    rng = np.random.default_rng(41)
    gms = [rng.standard_normal(pairs[0][0].shape).astype(np.float32) for _ in range(3)]
    alone = [run(device, enc, [pairs[i]], 1.0, g_out=[g[i]]) for i in range(3)]
    alone_m = [run(device, enc, [pairs[i]], 1.0, gmaps=[gms[i]], maps=False) for i in range(3)]
    check_against_float32(device, enc, pairs, 1.0, "the batch", g_out=g)
    for order in ((0, 1, 2), (2, 0, 1)):
        for again in range(2):
            s, ms, gr = run(device, enc, [pairs[i] for i in order], 1.0, g_out=[g[i] for i in order])
            _, _, gm = run(device, enc, [pairs[i] for i in order], 1.0, gmaps=[gms[i] for i in order], maps=False)
            for pos, i in enumerate(order):
                assert same64(s[pos:pos + 1], alone[i][0]) and HM.same_f32(ms[pos], alone[i][1][0]), (order, pos, again)
                for side in range(2):
                    assert np.array_equal(gr[pos][side], alone[i][2][0][side]) and np.array_equal(gm[pos][side], alone_m[i][2][0][side]), (order, pos, again)


@ENC
def test_deep_chunks_have_the_bits_of_the_lone_launch(device, enc):
    """17 x 17 x 131 in a launch of enough volumes that plan3f cuts z into chunks of at least 16 slices (a lone volume runs at 8): the
    planner changes neither sums nor maps nor gradients nor map gradients.  The first, a middle and the last volume of the deep launch
    get a map, each in a layout of its own (dense, step 2, negative sliceStride) over a sentinel prefill; the lone launch's value, sums
    and map are those of ssim3f on the widened volumes, through the enqueue, device and host entries."""
    w, h, d = shape = (17, 17, 131)
    assert P.plan3f(w, h, d, 1, device.cus).chunk_slices == P.CELL_Z
    n = next((n for n in range(2, 513) if P.plan3f(w, h, d, n, device.cus).chunk_slices >= 16), None)
    assert n is not None, "no launch of up to 512 volumes of 17 x 17 x 131 reaches chunks of 16 slices on %d CUs" % device.cus
    geo = P.plan3f(w, h, d, n, device.cus)
    print("on %d CUs: %s" % (device.cus, P.describe(geo, w, h, d, n)))
    assert geo.chunk_slices >= 16
    pairs = [IN.random_pair(shape, 50 + i, enc) for i in range(3)]
    gs = [0.75e4, -2.0e4, 0.5e4, 1.0e4]
    rng = np.random.default_rng(51)
    gms = [(rng.standard_normal(pairs[0][0].shape) * 10).astype(np.float32) for _ in range(2)]
    pick = [(i * 2 + i // 3) % 3 for i in range(n)]
    gpick = [(i * 3 + i // 4) % 4 for i in range(n)]
    mpick = [(i + i // 2) % 2 for i in range(n)]
    lone, lone_m, lone_fwd = {}, {}, []
    for k, pair in enumerate(pairs):
        for lmap in ("dense", "step 2", "negative sliceStride"):
            (fs, fms, _), _ = check_against_float32(device, enc, [pair], 1.0, ("lone forward", k, lmap), lmap=lmap)
        lone_fwd.append((fs, fms[0]))
    check_value_entries(device, enc, pairs[0], lone_fwd[0][0][0], lone_fwd[0][1])
    map_at = dict(zip(sorted(set((0, n // 2, n - 1))), ("dense", "step 2", "negative sliceStride")))
    assert len(map_at) == 3
    for i in range(n):
        if (pick[i], gpick[i]) not in lone:
            lone[(pick[i], gpick[i])], _ = check_against_float32(device, enc, [pairs[pick[i]]], 1.0, "lone", g_out=[gs[gpick[i]]], maps=False)
        if (pick[i], mpick[i]) not in lone_m:
            lone_m[(pick[i], mpick[i])] = run(device, enc, [pairs[pick[i]]], 1.0, gmaps=[gms[mpick[i]]], maps=False)
    s, ms, gr = run(device, enc, [pairs[k] for k in pick], 1.0, g_out=[gs[k] for k in gpick], maps=map_at)
    fs, fms, _ = run(device, None, widened([pairs[k] for k in pick], enc), 1.0, maps=map_at)      # ssim3f in the same deep launch
    assert same64(s, fs) and len(ms) == len(fms) == 3
    for i, m, fm in zip(sorted(map_at), ms, fms):
        assert HM.same_f32(m, lone_fwd[pick[i]][1]) and HM.same_f32(m, fm), "the map of volume %d (pair %d, %s) of the deep launch" % (i, pick[i], map_at[i])
    _, _, gm = run(device, enc, [pairs[k] for k in pick], 1.0, gmaps=[gms[k] for k in mpick], maps=False)
    for i in range(n):
        want, want_m = lone[(pick[i], gpick[i])], lone_m[(pick[i], mpick[i])]
        assert same64(s[i:i + 1], want[0]) and same64(s[i:i + 1], lone_fwd[pick[i]][0]), i
        for side in range(2):
            assert np.array_equal(gr[i][side], want[2][0][side]) and np.array_equal(gm[i][side], want_m[2][0][side]), (i, side)


def _dense_inputs(ctx, pairs):
    bufs = [(ctx.upload(a), ctx.upload(b)) for a, b in pairs]
    return bufs


@ENC
def test_enqueues_beyond_the_ring_keep_their_order(device, enc):
    """17 different pairs of 33 x 17 x 9: one forward and one gradient enqueue each, back to back -- 34 launches from the ring of 8
    descriptor slots -- and one synchronise: the lone results."""
    ctx, (w, h, d), n = device.ctx, (33, 17, 9), 17
    vox = w * h * d
    pairs = [IN.random_pair((w, h, d), 60 + i, enc) for i in range(n)]
    g_out = np.float32([(-0.75e4, 0.5e4, 1.0e4)[i % 3] for i in range(n)])
    lone = [run(device, enc, [pairs[i]], 1.0, g_out=[g_out[i]], maps=False) for i in range(n)]
    assert len(set(x[0].tobytes() for x in lone)) == n
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    bufs = _dense_inputs(ctx, pairs)
    per = vox + GAP
    fresh = np.full(2 * n * per + GAP, SENT[np.dtype(np.uint16)], np.uint16)
    out, sums, go = ctx.upload(fresh), ctx.upload(np.full(n + 2, -777.0)), ctx.upload(g_out)
    try:
        keep = []
        for i in range(n):
            ps, ga, gb = (ssim_amd.Params3H * 1)(), (ssim_amd.Grad3H * 1)(), (ssim_amd.Grad3H * 1)()
            ps[0] = ssim_amd.make_params3h(w, h, d, bufs[i][0].ptr, (1, w, w * h), bufs[i][1].ptr, (1, w, w * h))
            ga[0] = ssim_amd.Grad3H(out.ptr + 2 * (GAP + 2 * i * per), 1, w, w * h)
            gb[0] = ssim_amd.Grad3H(out.ptr + 2 * (GAP + (2 * i + 1) * per), 1, w, w * h)
            keep.append((ps, ga, gb))
            call(ctx.enqueue_ssim3h, ps, 1, 1.0, enc, sums.ptr + 8 * (1 + i))
            call(ctx.enqueue_ssim3h_grad, ps, 1, 1.0, enc, go.ptr + 4 * i, ga, gb)
        call(ctx.synchronize)
        device.sample()
        s = sums.download(np.float64, (n + 2,))
        assert s[0] == -777.0 and s[-1] == -777.0
        host = out.download(np.uint16, fresh.shape)
        body = host[GAP:].reshape(2 * n, per)
        assert np.all(host[:GAP] == fresh[0]) and np.all(body[:, vox:] == fresh[0]), "a gap between the gradient volumes changed"
        for i in range(n):
            assert same64(s[1 + i:2 + i], lone[i][0]), i
            for side in range(2):
                assert np.array_equal(body[2 * i + side, :vox].reshape(d, h, w), lone[i][2][0][side]), (i, side)
    finally:
        for x in [out, sums, go] + [b for ab in bufs for b in ab]:
            x.free()


@ENC
def test_a_call_beyond_the_launch_limit_is_cut_without_a_trace(device, enc):
    """65537 volumes of 2 x 1 x 3 in one forward and one gradient call: sub-batches of 65535 and 2 volumes; drawn from 5 pairs x 3 gOut
    values, neighbours differing; every volume has the bits of its combination launched alone."""
    ctx, (w, h, d), n = device.ctx, (2, 1, 3), 65537
    vox, npairs, ngs = w * h * d, 5, 3
    for scratch in (P.forward_scratch(w, h, d), P.grad_scratch(w, h, d, 3)):
        assert P.sub_batches(w, h, d, n, scratch) == [(0, 65535), (65535, 2)]
    pairs = [IN.random_pair((w, h, d), 70 + i, enc) for i in range(npairs)]
    gs = np.float32([-30.0, 12.0, 50.0])
    combo = np.random.default_rng([20261019, n]).permutation(np.arange(n) % (npairs * ngs))
    pick, gpick = combo % npairs, combo % ngs
    assert len(set(zip(pick.tolist(), gpick.tolist()))) == npairs * ngs
    sums_alone, grads_alone = np.zeros(npairs), np.zeros((npairs, ngs, 2, vox), np.uint16)
    for k in range(npairs):
        for g in range(ngs):
            (s, _, gr), _ = check_against_float32(device, enc, [pairs[k]], 1.0, "alone", g_out=[gs[g]], maps=False)
            sums_alone[k] = s[0]
            grads_alone[k, g, 0], grads_alone[k, g, 1] = gr[0][0].reshape(-1), gr[0][1].reshape(-1)
    assert len(set(grads_alone[k, g].tobytes() for k in range(npairs) for g in range(ngs))) == npairs * ngs
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    bufs = _dense_inputs(ctx, pairs)
    per = vox + 2
    fresh = np.full(2 * n * per + 2, SENT[np.dtype(np.uint16)], np.uint16)
    out, sm, go = ctx.upload(fresh), ctx.upload(np.full(n + 2, -777.0)), ctx.upload(gs[gpick])
    try:
        ps, ga, gb = (ssim_amd.Params3H * n)(), (ssim_amd.Grad3H * n)(), (ssim_amd.Grad3H * n)()
        one = (ssim_amd.Params3H * npairs)(*[ssim_amd.make_params3h(w, h, d, bufs[k][0].ptr, (1, w, w * h), bufs[k][1].ptr, (1, w, w * h)) for k in range(npairs)])
        np.frombuffer(ps, np.dtype(ssim_amd.Params3H))[:] = np.frombuffer(one, np.dtype(ssim_amd.Params3H))[pick]
        for side, arr in enumerate((ga, gb)):
            gv = np.frombuffer(arr, np.dtype(ssim_amd.Grad3H))
            gv["topLeft"] = out.ptr + 2 * (2 + (2 * np.arange(n, dtype=np.uint64) + side) * per)
            gv["step"], gv["stride"], gv["sliceStride"] = 1, w, w * h
        assert ps[n - 1].imgA.topLeft == bufs[pick[n - 1]][0].ptr and gb[n - 1].topLeft + 2 * vox + 4 == out.ptr + fresh.nbytes
        call(ctx.enqueue_ssim3h, ps, n, 1.0, enc, sm.ptr + 8)
        call(ctx.enqueue_ssim3h_grad, ps, n, 1.0, enc, go.ptr, ga, gb)
        call(ctx.synchronize)
        device.sample()
        s = sm.download(np.float64, (n + 2,))
        assert s[0] == -777.0 and s[-1] == -777.0, "a double beside the sums was written"
        bad = np.flatnonzero(s[1:-1].view(np.uint64) != sums_alone[pick].view(np.uint64))
        assert len(bad) == 0, "%d of %d fp64 sums differ from the volume launched alone; the first: volume %d" % (len(bad), n, bad[0])
        host = out.download(np.uint16, fresh.shape)
        body = host[2:].reshape(2 * n, per)
        assert np.all(host[:2] == fresh[0]) and np.all(body[:, vox:] == fresh[0]), "a gap between the gradient volumes changed"
        bad = np.flatnonzero(np.any(body[:, :vox].reshape(n, 2 * vox) != grads_alone[pick, gpick].reshape(n, 2 * vox), axis=1))
        assert len(bad) == 0, "the gradients of %d of %d volumes differ from the ones of the volume launched alone; the first: volume %d" % (len(bad), n, bad[0])
    finally:
        for x in [out, sm, go] + [b for ab in bufs for b in ab]:
            x.free()


# ---- the float64 model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(6))
def test_stored_golden_volumes_against_the_float64_model(device, manifest, i):
    """Value, map and sums of the golden-derived volumes, as stored in each encoding, at ssim3f_model.tolerances() (the input condition:
    tests/test_ssim3h_cpu.py); the gradient is held through the bit identity alone -- the float64 model does not round to 16 bits."""
    px_tol, g_tol, _, _ = S.tolerances()
    what, enc, ua, ub, r = IN.golden_cases(manifest)[i]
    gv, gm = IN.golden_model(manifest, i)
    g = normal_scale(device, enc, (ua, ub), r)
    (s, ms, _), _ = check_against_float32(device, enc, [(ua, ub)], r, what, g_out=[g])
    dv, dp = abs(s[0] / S.voxels(ua.shape) - gv), float(np.abs(ms[0].astype(np.float64) - gm).max())
    print("%s: per voxel %.3g (bound %.3g), global %.3g (bound %.3g)" % (what, dp, px_tol, dv, g_tol))
    assert dp <= px_tol and dv <= g_tol, (what, dp, dv)


# ---- PyTorch -------------------------------------------------------------------------------------------------------------------------
# torch brings its own HIP runtime; the checks run in ONE child process (tests/tools/ssim3h_torch_checks.py) that imports torch before the
# library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    tool = os.path.join(ROOT, "tests", "tools", "ssim3h_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "ssim3h_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["forward_and_backward_are_the_c_abi", "non_contiguous_and_expanded_inputs_are_read_in_place", "loss_under_autocast",
                                   "loss_scale_arrives_before_the_rounding", "masked_map_loss", "mixed_pairs_are_refused", "side_stream"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
