"""GPU: one training step's mix of SSIM calls on ONE context, held to each call alone.

Why.  Every sample family (ssim16, ssimf, the windowed ssimf, ssimh, msssimf, msssimh, the volume family ssim3f and their gradients) takes its descriptor tables from
one ring of 8 slots, writes its cell partials into one buffer and -- the two multi-scale families -- rebuilds its pyramid, its coarse
gradient planes and its coefficients in one set of grow-only buffers whose grow() frees before it allocates (ssim_context.h: "Every family
shares them: one stream, stream order").  The other modules drive one family at a time with a synchronise after every call or two.  Here a
sequence of 61 enqueues of every asynchronous sample entry, forwards and backwards, of four shapes and 1 .. 8 pairs and of two volume shapes, goes onto one context
back to back without a host wait; one synchronise and one read-back follow.

What is asserted.  Every byte of every output buffer of the sequence -- fp64 sums, maps, values, per-scale means, gradient planes, the
sentinel gaps of interleaved planes and the sentinel elements around every fp64 vector included -- equals the byte the same op, on the
same pixels in the same layouts, leaves when it is issued ALONE on a second context that is synchronised after every op.  No tolerance:
both sides run the same kernels on the same pixels.  So that "the same wrong bits on both sides" is excluded, the lone results of at least
one pair per family are held to the float64 models at the bounds the families' own modules assert (ssim16_model, ssimf_model, ssimw_model,
ssimk_model.tolerances, msssimf_model, ssim3f_model.tolerances; the 16-bit encodings: the bits of the float32 entries on the planes widened by halfmodel, rounded
once for the gradients).  No bound is new.

The sequence (Sequence.build).  Sizes are W x H: 33 x 17 with 1 to 3 pairs, 130 x 19 (two strip columns, map rows of 520 bytes: no
multiple of 64), the 257 x 65 golden pairs / 255, and 8 pairs (ssimf) / 4 pairs (msssimf, msssimh and the backward) of 512 x 512, which
regrow every shared buffer after smaller launches used it and keep the stream busy while the host issues what follows.  One uint8
enqueue_batch of two golden fixtures shares only the stream.  Every multi-scale forward F whose means a backward consumes is followed,
BEFORE that backward, by a forward of other pairs of the same shape and count, one of the same family at another shape and one of the
other multi-scale family at F's shape and count: the backward must rebuild its own pyramid.  ssimf of one 33 x 17 pair is issued twice,
first and last, into different outputs: the same bits.  The volume family (W x H x D) shares the ring and the cell partials and adds a
coefficient scratch of its own: enqueue_ssim3f with maps (dense, and two floats apart) and enqueue_ssim3f_grad for both gradients and for
one, on 3 pairs and on 1 pair of 33 x 20 x 13 and on 2 pairs of 65 x 63 x 40, which regrow the cell partials and the coefficient scratch after
smaller work; the backward of the 3 pairs follows a 2-D launch of more cells than its forward has (a gradient enqueue puts two tables in
one ring slot).

Orders: ascending size (every shared buffer is regrown while earlier work is queued), descending size (small launches run in scratch
that holds a larger launch's partials, pyramid and gradient planes) and a seeded shuffle; all three keep every op after the ops it names
(a backward after its forward and after the forwards that must lie between).  Every forward and then every backward, both ascending,
with trim() after each third (every backward then follows a trim that its forward preceded), then on the trimmed context once more; and the ops split into two dependency-closed halves issued alternately on two contexts with
streams of their own.

After a return code that is neither success nor EINVAL the module starts nothing more on the GPU (test_gpu_ssimk's _device_error, shared
with that module).  Every test frees its own buffers.  The module prints its wall time and its peak device memory when it ends.

Cost, measured on an MI355X: the 9 tests take 4.3 s together (3.1 s of it the torch child process, 0.5 s the lone calls and their float64
models), no test more than 0.1 s of its own; the device holds 96 MiB more than before the module at the peak.
"""
import json
import os
import subprocess
import sys
import time
import traceback

import numpy as np
import pytest

import halfmodel as HM
import msssimf_model as MS
import sample_forms_inputs as IN
import ssim16_model as M16
import ssim3f_model as S3
import ssimf_model as MF
import ssimk_model as K
import ssimw_model as MW
import ssim_amd
from conftest import ROOT, load_pair
from test_gpu_ssim16 import G_TOL as G16_TOL, PX_TOL as PX16_TOL
from test_gpu_ssim3f import random_pair as random_volumes
from test_gpu_ssimk import _device_error, mk
from test_gpu_ssimw import FILL16, FILL32, Plane

pytestmark = pytest.mark.gpu

RANGE = IN.RANGE
FILL64 = np.float64(-777.0)
SMALL, TWOCOL, GOLD, BIG = (17, 33), (19, 130), (65, 257), (512, 512)          # (H, W)
GOLDEN = ("bbb257x65_q50_ch1", "bbb257x65_q00_ch1")
WIN7U, WIN5G = (7, 0.0, "uniform"), (5, 0.8, "gaussian")                       # two of ssimk_model.WINDOWS
MS5, MS3 = (5, None), (3, (0.2, 0.3, 0.5))                                      # Wang's five; three scales, weights of its own
DENSE, WIDE3, BACK, BACK2 = (1, False), (3, False), (1, True), (2, True)       # (step, flip) of test_gpu_ssimw.Plane
VOL, VOLBIG = (33, 20, 13), (65, 63, 40)                                       # W x H x D of the volume ops
SHUFFLE_SEED = 20261019
assert WIN7U in K.WINDOWS and WIN5G in K.WINDOWS


# ---- inputs: seeded, drawn once ---------------------------------------------------------------------------------------------------------

_inputs = {}


def _rng(shape, salt):
    return np.random.default_rng([IN.SEED, shape[0], shape[1], salt])


def pairs_f(shape, n, salt):
    """n float32 pairs in [0, 1] (sample_forms_inputs.random_pair_f)."""
    key = ("f", shape, n, salt)
    if key not in _inputs:
        rng = _rng(shape, salt)
        _inputs[key] = [IN.random_pair_f(shape[0], shape[1], rng) for _ in range(n)]
    return _inputs[key]


def pairs_16(shape, n, salt, depth):
    key = ("16", shape, n, salt, depth)
    if key not in _inputs:
        _inputs[key] = IN.pairs16(_rng(shape, salt), n, shape, depth)
    return _inputs[key]


def pairs_h(shape, n, salt, enc):
    """([(bit patterns a, b)], [(the float32 planes they stand for)])."""
    key = ("h", shape, n, salt, enc)
    if key not in _inputs:
        rng = _rng(shape, salt)
        got = [IN.random_pair_h(shape[0], shape[1], rng, enc) for _ in range(n)]
        _inputs[key] = ([u for u, _ in got], [f for _, f in got])
    return _inputs[key]


def pairs_3f(size, n, salt):
    """n float32 pairs of volumes in [0, 1], (D, H, W) arrays (test_gpu_ssim3f.random_pair)."""
    key = ("3f", size, n, salt)
    if key not in _inputs:
        _inputs[key] = [random_volumes(size, IN.SEED + 1000 * salt + i) for i in range(n)]
    return _inputs[key]


def golden_f(manifest, name):
    a, b = load_pair(manifest[name])
    return a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)


def upstream(shape, n, salt):
    """n per-pixel upstream gradients: seeded standard normal planes (ssimw_model.weight_planes / ssimk_model.upstream_planes, "normal")."""
    return [dict(MW.weight_planes(shape[0], shape[1], seed=salt + i))["normal"] for i in range(n)]


# ---- outputs and ops ----------------------------------------------------------------------------------------------------------------------

class Out(object):
    """One output buffer of an op, pre-filled with a sentinel: `host` is what it holds before the op, `owned` the elements the op writes."""

    def __init__(self, mem, name, host, owned, ptr_offset=0):
        self.name, self.init, self.owned = name, host, owned
        self.buf = mem.upload(host)
        self.ptr = self.buf.ptr + ptr_offset

    def read(self):
        return self.buf.download(self.init.dtype, self.init.shape)

    def free(self):
        self.buf.free()


class PlaneOut(Out):
    """An H x W output plane in a layout of test_gpu_ssimw.Plane: samples `step` apart with sentinels between them, and / or stored back
    to front behind negative steps."""

    def __init__(self, mem, name, h, w, dtype, lay):
        fill = FILL32 if dtype == np.float32 else FILL16
        p = Plane(mem, np.full((h, w), fill, dtype), step=lay[0], flip=lay[1], fill=fill)
        self.name, self.buf, self.ptr, self.dstep, self.dstride, self.lay = name, p.buf, p.ptr, p.dstep, p.dstride, lay
        self.init = np.full((h, w, lay[0]), fill, dtype)
        self.owned = np.zeros(self.init.shape, bool)
        self.owned[:, :, lay[0] - 1] = True

    def plane(self, host):
        p = host[:, :, self.lay[0] - 1]
        return np.ascontiguousarray(p[::-1, ::-1] if self.lay[1] else p)


class VolOut(Out):
    """A D x H x W output volume: samples `step` elements apart with sentinels between them; float32, or uint16 (a 16-bit gradient)."""

    def __init__(self, mem, name, d, h, w, step=1, dtype=np.float32):
        fill = FILL32 if dtype == np.float32 else FILL16
        owned = np.zeros((d, h, w, step), bool)
        owned[..., step - 1] = True
        Out.__init__(self, mem, name, np.full((d, h, w, step), fill, dtype), owned, ptr_offset=np.dtype(dtype).itemsize * (step - 1))
        self.strides = (step, step * w, step * w * h)            # step, stride, sliceStride

    def plane(self, host):
        return np.ascontiguousarray(host[..., -1])


class VecOut(Out):
    """n doubles with one sentinel double before and one after them."""

    def __init__(self, mem, name, n):
        owned = np.zeros(n + 2, bool)
        owned[1:n + 1] = True
        Out.__init__(self, mem, name, np.full(n + 2, FILL64), owned, ptr_offset=8)

    def vec(self, host):
        return host[1:-1]


class Op(object):
    """One enqueue call on a context and the sentinel-filled device buffers it writes."""

    def __init__(self, name, entry, shape, n, note, call, outs, keep, after=()):
        self.name, self.entry, self.shape, self.n, self.note = name, entry, shape, n, note
        self.call, self.outs, self.keep, self.after = call, outs, keep, list(after)
        self.size = shape[0] * shape[1] * n
        self.at = None                                           # position in Sequence.ops

    def issue(self, ctx):
        """Any return code other than 0 stops the sequence at once (SsimError); one that is neither 0 nor EINVAL is a device error."""
        assert not _device_error, "an earlier call left a device error: %r" % _device_error
        try:
            self.call(ctx)
        except ssim_amd.SsimError as e:
            if e.errno != 22:
                _device_error.append(e.errno)
            raise

    def read(self):
        return dict((o.name, o.read().tobytes()) for o in self.outs)

    def describe(self):
        return "%-14s %-28s %3d x %-3d x %d  %s" % (self.name, self.entry, self.shape[1], self.shape[0], self.n, self.note)


def _sync(ctx):
    try:
        ctx.synchronize()
    except ssim_amd.SsimError as e:
        _device_error.append(e.errno)
        raise


class Sequence(object):
    """The ops of the mixed step over buffers of their own (allocated through `mem`, a context that issues none of them)."""

    def __init__(self, mem, manifest):
        self.mem, self.manifest, self.ops, self.by_name, self.bufs = mem, manifest, [], {}, []
        try:
            self.build()
        except Exception:
            self.free()
            raise

    def free(self):
        for op in self.ops:
            for x in op.outs + op.keep:
                x.free()
        for b in self.bufs:
            b.free()
        self.ops, self.bufs = [], []

    def add(self, op):
        assert op.name not in self.by_name
        op.at = len(self.ops)
        self.ops.append(op)
        self.by_name[op.name] = op
        return op

    # -- the single-scale entries --

    def forward(self, name, kind, pairs, lay=DENSE, maps=None, after=(), planes_of=None, **kw):
        """kind "16" (depth), "f", "k" (window), "h" (enc); maps: the pairs that get a map (None: all); planes_of: the forward op whose
        device planes of the same pairs are read (the outputs are this op's own)."""
        mem, n, (h, w) = self.mem, len(pairs), pairs[0][0].shape
        small = kind in ("16", "h")
        ps = ((ssim_amd.Params16 if small else ssim_amd.ParamsF) * n)()
        make = ssim_amd.make_params16 if small else ssim_amd.make_params_f
        keep, outs = [], []
        for i, (a, b) in enumerate(pairs):
            if planes_of is None:
                pa, pb = Plane(mem, a, step=lay[0], flip=lay[1]), Plane(mem, b, step=lay[0], flip=lay[1])
                keep += [pa, pb]
            else:
                assert planes_of.pairs is pairs and planes_of.lay == lay
                pa, pb = planes_of.keep[2 * i], planes_of.keep[2 * i + 1]
            args = (w, h, pa.ptr, pa.dstep, pa.dstride, pb.ptr, pb.dstep, pb.dstride)
            if maps is None or i in maps:
                m = PlaneOut(mem, "map%d" % i, h, w, np.float32, lay)
                outs.append(m)
                args += (m.ptr, m.dstep, m.dstride)
            ps[i] = make(*args)
        sums = VecOut(mem, "sums", n)
        outs.append(sums)
        if kind == "16":
            entry, call = "enqueue_ssim16", lambda ctx: ctx.enqueue_ssim16(ps, n, kw["depth"], sums.ptr)
        elif kind == "f":
            entry, call = "enqueue_ssimf", lambda ctx: ctx.enqueue_ssimf(ps, n, RANGE, sums.ptr)
        elif kind == "k":
            win = mk(kw["window"])
            entry, call = "enqueue_ssimf_win", lambda ctx: ctx.enqueue_ssimf(ps, n, RANGE, sums.ptr, window=win)
        else:
            entry, call = "enqueue_ssimh", lambda ctx: ctx.enqueue_ssimh(ps, n, RANGE, kw["enc"], sums.ptr)
        note = "%s, layout %r, %d maps" % (kw.get("depth") or kw.get("enc") or K.name_of(kw.get("window", K.DEFAULT)), lay, len(outs) - 1)
        op = self.add(Op(name, entry, (h, w), n, note, call, outs, keep, after))
        op.kind, op.kw, op.params, op.pairs, op.lay = kind, kw, ps, pairs, lay
        return op

    def grad_planes(self, n, h, w, which, half, lay):
        cls, dt = (ssim_amd.GradH, np.uint16) if half else (ssim_amd.GradF, np.float32)
        arrs, outs = [None, None], []
        for k in range(2):
            if which & (1 << k):
                arrs[k] = (cls * n)()
                for i in range(n):
                    g = PlaneOut(self.mem, "d%s%d" % ("AB"[k], i), h, w, dt, lay)
                    outs.append(g)
                    arrs[k][i] = cls(g.ptr, g.dstep, g.dstride)
        return arrs, outs

    def backward(self, name, f, form, which=3, lay=DENSE, salt=0, g_out=None):
        """The gradient of the forward op f's pairs: form "scalar" (g_out per pair; default: G_OUT times 1, 1.5, 2 ...) or "map" (a seeded
        upstream plane per pair)."""
        mem, n, (h, w), half = self.mem, f.n, f.shape, f.kind == "h"
        ps = f.params
        arrs, outs = self.grad_planes(n, h, w, which, half, lay)
        win = mk(f.kw["window"]) if f.kind == "k" else None
        keep = []
        if form == "scalar":
            # 16-bit planes: W H, so that the rounded pixels are normal numbers (sample_forms_inputs.g_out_h)
            if g_out is None:
                g_out = np.float32([(IN.g_out_h(h, w) if half else IN.G_OUT) * (1.0 + 0.5 * i) for i in range(n)])
            go = mem.upload(g_out)
            keep.append(go)
            if half:
                entry, call = "enqueue_ssimh_grad", lambda ctx: ctx.enqueue_ssimh_grad(ps, n, RANGE, f.kw["enc"], go.ptr, arrs[0], arrs[1])
            elif win is None:
                entry, call = "enqueue_ssimf_grad", lambda ctx: ctx.enqueue_ssimf_grad(ps, n, RANGE, go.ptr, arrs[0], arrs[1])
            else:
                entry, call = "enqueue_ssimf_win_grad", lambda ctx: ctx.enqueue_ssimf_grad(ps, n, RANGE, go.ptr, arrs[0], arrs[1], window=win)
            up = g_out
        else:
            up = upstream((h, w), n, salt)
            ms = (ssim_amd.GradOutF * n)()
            for i in range(n):
                m = Plane(mem, up[i], step=lay[0], flip=lay[1])
                keep.append(m)
                ms[i] = ssim_amd.GradOutF(m.ptr, m.dstep, m.dstride)
            if half:
                entry, call = "enqueue_ssimh_map_grad", lambda ctx: ctx.enqueue_ssimh_map_grad(ps, n, RANGE, f.kw["enc"], ms, arrs[0], arrs[1])
            elif win is None:
                entry, call = "enqueue_ssimf_map_grad", lambda ctx: ctx.enqueue_ssimf_map_grad(ps, n, RANGE, ms, arrs[0], arrs[1])
            else:
                entry, call = "enqueue_ssimf_win_map_grad", lambda ctx: ctx.enqueue_ssimf_map_grad(ps, n, RANGE, ms, arrs[0], arrs[1], window=win)
        note = "of %s, %s, layout %r" % (f.name, ("dA", "dB", "dA dB")[which - 1], lay)
        op = self.add(Op(name, entry, (h, w), n, note, call, outs, keep, [f]))
        op.of, op.form, op.which, op.up, op.salt = f, form, which, up, salt
        return op

    # -- the multi-scale entries --

    def ms_forward(self, name, pairs, config, enc=None, lay=DENSE, after=()):
        mem, n, (h, w) = self.mem, len(pairs), pairs[0][0].shape
        scales, weights = config
        ps = ((ssim_amd.Params16 if enc else ssim_amd.ParamsF) * n)()
        make = ssim_amd.make_params16 if enc else ssim_amd.make_params_f
        keep = []
        for i, (a, b) in enumerate(pairs):
            pa, pb = Plane(mem, a, step=lay[0], flip=lay[1]), Plane(mem, b, step=lay[0], flip=lay[1])
            keep += [pa, pb]
            ps[i] = make(w, h, pa.ptr, pa.dstep, pa.dstride, pb.ptr, pb.dstep, pb.dstride)
        values, means = VecOut(mem, "values", n), VecOut(mem, "means", n * scales * 2)
        if enc:
            entry, call = "enqueue_msssimh", lambda ctx: ctx.enqueue_msssimh(ps, n, RANGE, enc, values.ptr, means.ptr, scales, weights)
        else:
            entry, call = "enqueue_msssimf", lambda ctx: ctx.enqueue_msssimf(ps, n, RANGE, values.ptr, means.ptr, scales, weights)
        note = "%s%d scales, layout %r" % (enc + ", " if enc else "", scales, lay)
        op = self.add(Op(name, entry, (h, w), n, note, call, [values, means], keep, after))
        op.kind, op.enc, op.config, op.params, op.pairs, op.means = "msh" if enc else "ms", enc, config, ps, pairs, means
        return op

    def ms_backward(self, name, f, which, between, lay=DENSE, g_out=None):
        """The backward of the multi-scale forward f from f's own means buffer, after every forward of `between`."""
        mem, n, (h, w), half = self.mem, f.n, f.shape, f.enc is not None
        ps, (scales, weights), means = f.params, f.config, f.means
        arrs, outs = self.grad_planes(n, h, w, which, half, lay)
        if g_out is None:
            g_out = np.float32([(IN.g_out_h(h, w) if half else IN.G_OUT) * (1.0 + 0.5 * i) for i in range(n)])
        go = mem.upload(g_out)
        if half:
            entry, call = "enqueue_msssimh_grad", lambda ctx: ctx.enqueue_msssimh_grad(ps, n, RANGE, f.enc, means.ptr, go.ptr, arrs[0], arrs[1], scales, weights)
        else:
            entry, call = "enqueue_msssimf_grad", lambda ctx: ctx.enqueue_msssimf_grad(ps, n, RANGE, means.ptr, go.ptr, arrs[0], arrs[1], scales, weights)
        note = "of %s, %s, after %s" % (f.name, ("dA", "dB", "dA dB")[which - 1], " ".join(b.name for b in between))
        op = self.add(Op(name, entry, (h, w), n, note, call, outs, [go], [f] + list(between)))
        op.of, op.which, op.up, op.between = f, which, g_out, list(between)
        return op

    def ms_group(self, tag, pairs, others, config, which, enc=None, lay=DENSE, glay=DENSE):
        """A multi-scale forward, its backward, and between the two: the same entry on other pairs of the same shape and count, the same
        family at another shape (one pair) and the other family at the same shape and count (other pairs again)."""
        (h, w), n = pairs[0][0].shape, len(pairs)
        f = self.ms_forward(tag, pairs, config, enc, lay)
        same_shape = self.ms_forward(tag + ".same", others, config, enc, lay, after=[f])
        oshape = TWOCOL if (h, w) == SMALL else SMALL
        if enc:
            at_other_shape = self.ms_forward(tag + ".shape", pairs_h(oshape, 1, 900 + len(self.ops), enc)[0], config, enc, after=[f])
            other_family = self.ms_forward(tag + ".family", pairs_f((h, w), n, 900 + len(self.ops)), MS5, after=[f])
        else:
            at_other_shape = self.ms_forward(tag + ".shape", pairs_f(oshape, 1, 900 + len(self.ops)), config, after=[f])
            other_family = self.ms_forward(tag + ".family", pairs_h((h, w), n, 900 + len(self.ops), HM.BF16)[0], MS3, HM.BF16, after=[f])
        return f, self.ms_backward(tag + ".grad", f, which, [same_shape, at_other_shape, other_family], glay)

    # -- the volume family: the ring, the cell partials and a coefficient scratch of its own --

    def vol_forward(self, name, pairs, maps=None, step=1, after=()):
        """enqueue_ssim3f of `pairs` ((D, H, W) arrays, dense in device memory); maps: the pairs that get a map (None: all), `step`
        floats apart."""
        mem, n, (d, h, w) = self.mem, len(pairs), pairs[0][0].shape
        ps = (ssim_amd.Params3F * n)()
        keep, outs = [], []
        for i, (a, b) in enumerate(pairs):
            da, db = mem.upload(a), mem.upload(b)
            keep += [da, db]
            m = None
            if maps is None or i in maps:
                m = VolOut(mem, "map%d" % i, d, h, w, step)
                outs.append(m)
            ps[i] = ssim_amd.make_params3f(w, h, d, da.ptr, (1, w, w * h), db.ptr, (1, w, w * h), m.ptr if m else None, m.strides if m else None)
        sums = VecOut(mem, "sums", n)
        outs.append(sums)
        note = "depth %d, %d maps, step %d" % (d, len(outs) - 1, step)
        op = self.add(Op(name, "enqueue_ssim3f", (h, w), n, note, lambda ctx: ctx.enqueue_ssim3f(ps, n, RANGE, sums.ptr), outs, keep, after))
        op.kind, op.params, op.pairs, op.depth = "3f", ps, pairs, d
        op.size *= d
        return op

    def vol_backward(self, name, f, which=3, step=1, after=()):
        """enqueue_ssim3f_grad of the volume forward f's pairs, after f and the ops of `after`."""
        mem, n, (h, w), d = self.mem, f.n, f.shape, f.depth
        arrs, outs = [None, None], []
        for k in range(2):
            if which & (1 << k):
                arrs[k] = (ssim_amd.Grad3F * n)()
                for i in range(n):
                    g = VolOut(mem, "d%s%d" % ("AB"[k], i), d, h, w, step)
                    outs.append(g)
                    arrs[k][i] = ssim_amd.Grad3F(g.ptr, *g.strides)
        g_out = np.float32([IN.G_OUT * (1.0 + 0.5 * i) for i in range(n)])
        go = mem.upload(g_out)
        note = "of %s, %s, depth %d, step %d" % (f.name, ("dA", "dB", "dA dB")[which - 1], d, step)
        op = self.add(Op(name, "enqueue_ssim3f_grad", (h, w), n, note,
                         lambda ctx: ctx.enqueue_ssim3f_grad(f.params, n, RANGE, go.ptr, arrs[0], arrs[1]), outs, [go], [f] + list(after)))
        op.of, op.which, op.up = f, which, g_out
        op.size *= d
        return op

    # -- the uint8 engine: shares only the stream --

    def batch8(self, name):
        mem = self.mem
        keep, outs = [], []
        ps = (ssim_amd.Params * len(GOLDEN))()
        for i, g in enumerate(GOLDEN):
            a, b = load_pair(self.manifest[g])
            (h, w), da, db = a.shape, mem.upload(a), mem.upload(b)
            self.bufs += [da, db]
            m = PlaneOut(mem, "map%d" % i, h, w, np.float32, DENSE)
            outs.append(m)
            ps[i] = ssim_amd.make_params(w, h, da.ptr, 1, w, db.ptr, 1, w, m.ptr, 1, w)
        sums = VecOut(mem, "sums", len(GOLDEN))
        outs.append(sums)
        op = self.add(Op(name, "enqueue_batch", (h, w), len(GOLDEN), "uint8, two golden fixtures, 2 maps", lambda ctx: ctx.enqueue_batch(ps, len(GOLDEN), sums.ptr), outs, keep))
        op.kind = "8"
        return op

    def build(self):
        gold = [golden_f(self.manifest, g) for g in GOLDEN]
        F16, BF16 = HM.F16, HM.BF16
        # the same pairs (the same device planes) twice, first and last, into different outputs
        first = self.forward("ssimf.first", "f", pairs_f(SMALL, 1, 1))
        # ssim16, depth 10, with maps
        self.forward("ssim16.small", "16", pairs_16(SMALL, 3, 2, 10), depth=10)
        self.forward("ssim16.twocol", "16", pairs_16(TWOCOL, 2, 3, 10), lay=WIDE3, depth=10)
        # ssimf and its two gradients
        f_small = self.forward("ssimf.small", "f", pairs_f(SMALL, 3, 4), lay=BACK)
        f_two = self.forward("ssimf.twocol", "f", pairs_f(TWOCOL, 2, 5))
        f_gold = self.forward("ssimf.gold", "f", gold, lay=WIDE3)
        self.forward("ssimf.big", "f", pairs_f(BIG, 8, 6), maps=(0, 7))
        self.backward("ssimf.small.g", f_small, "scalar", lay=BACK)
        self.backward("ssimf.gold.g", f_gold, "scalar", which=1)
        self.backward("ssimf.twocol.m", f_two, "map", lay=WIDE3, salt=10)
        self.backward("ssimf.small.m", f_small, "map", which=2, salt=20)
        # the two windows: forward, gradient, map gradient
        u_two = self.forward("win7u.twocol", "k", pairs_f(TWOCOL, 2, 7), window=WIN7U)
        u_small = self.forward("win7u.small", "k", pairs_f(SMALL, 3, 8), lay=BACK2, window=WIN7U)
        g_gold = self.forward("win5g.gold", "k", gold[:1], window=WIN5G)
        g_two = self.forward("win5g.twocol", "k", pairs_f(TWOCOL, 1, 9), lay=WIDE3, window=WIN5G)
        self.backward("win7u.twocol.g", u_two, "scalar")
        self.backward("win5g.twocol.g", g_two, "scalar", which=2, lay=WIDE3)
        self.backward("win7u.small.m", u_small, "map", lay=BACK2, salt=30)
        self.backward("win5g.gold.m", g_gold, "map", which=1, salt=40)
        # ssimh in both encodings: forward, gradient, map gradient
        h_two = self.forward("ssimh.f16.twocol", "h", pairs_h(TWOCOL, 2, 11, F16)[0], enc=F16)
        h_small = self.forward("ssimh.f16.small", "h", pairs_h(SMALL, 1, 12, F16)[0], lay=WIDE3, enc=F16)
        b_small = self.forward("ssimh.bf16.small", "h", pairs_h(SMALL, 2, 13, BF16)[0], lay=BACK, enc=BF16)
        b_gold = self.forward("ssimh.bf16.gold", "h", [(HM.round_to(gold[0][0], BF16), HM.round_to(gold[0][1], BF16))], enc=BF16)
        self.backward("ssimh.f16.twocol.g", h_two, "scalar")
        self.backward("ssimh.bf16.small.g", b_small, "scalar", which=1, lay=BACK)
        self.backward("ssimh.f16.small.m", h_small, "map", lay=WIDE3, salt=50)
        self.backward("ssimh.bf16.gold.m", b_gold, "map", which=2, salt=60)
        # the multi-scale families: msssimf at Wang's five scales, msssimh at three scales of its own weights; one gradient and both
        self.ms_group("msf.twocol", pairs_f(TWOCOL, 2, 14), pairs_f(TWOCOL, 2, 15), MS5, which=3, glay=WIDE3)
        self.ms_group("msf.gold", gold[:1], gold[1:], MS5, which=1, lay=BACK)
        self.ms_group("msf.big", pairs_f(BIG, 4, 16), pairs_f(BIG, 4, 17), MS5, which=3)
        self.ms_group("msh.f16.twocol", pairs_h(TWOCOL, 2, 18, F16)[0], pairs_h(TWOCOL, 2, 19, F16)[0], MS3, which=2, enc=F16)
        self.ms_group("msh.bf16.small", pairs_h(SMALL, 3, 20, BF16)[0], pairs_h(SMALL, 3, 21, BF16)[0], MS3, which=3, enc=BF16, lay=WIDE3, glay=BACK)
        # the volume family: 33 x 20 x 13 with 3 pairs and with 1, and 2 pairs of 65 x 63 x 40, which regrow the cell partials and the
        # coefficient scratch after the smaller volumes; between vol.small and its backward a 2-D launch of more cells than vol.small has
        v_small = self.vol_forward("vol.small", pairs_3f(VOL, 3, 22))
        regrow = self.forward("ssimf.regrow", "f", pairs_f(GOLD, 1, 23), after=[v_small])
        v_one = self.vol_forward("vol.one", pairs_3f(VOL, 1, 24), step=2)
        v_big = self.vol_forward("vol.big", pairs_3f(VOLBIG, 2, 25), maps=(1,))
        self.vol_backward("vol.small.g", v_small, after=[regrow])
        self.vol_backward("vol.one.g", v_one, which=2, step=2)
        self.vol_backward("vol.big.g", v_big, which=1)
        self.batch8("batch8")
        last = self.forward("ssimf.last", "f", pairs_f(SMALL, 1, 1), planes_of=first)
        self.twins = (first, last)
        ring = [op for op in self.ops if op.entry != "enqueue_batch"]      # every sample entry here is one launch from the ring of 8 tables
        assert len(ring) >= 2 * 8 + 1 and len(set((op.entry, op.n) for op in ring)) >= 24      # tables of many sizes


# ---- orders -------------------------------------------------------------------------------------------------------------------------------

def order_of(ops, how, seed=SHUFFLE_SEED, twins=(), phases=False):
    """A topological order of `ops` (every op after the ops of its `after` that are in `ops`): "ascending" / "descending" take the
    smallest / largest ready op next (pixels x pairs; ties in list order), "shuffle" a seeded random one.  twins: the two ops that
    stay first and last; phases: every forward, then every backward, as a training step has them."""
    if twins:
        return [twins[0]] + order_of([op for op in ops if op not in twins], how, seed, phases=phases) + [twins[1]]
    if phases:
        return order_of([op for op in ops if not hasattr(op, "of")], how, seed) + order_of([op for op in ops if hasattr(op, "of")], how, seed)
    inside = set(op.at for op in ops)
    waits = dict((op.at, set(a.at for a in op.after if a.at in inside)) for op in ops)
    rng = np.random.default_rng(seed)
    done, out, left = set(), [], list(ops)
    while left:
        ready = [op for op in left if waits[op.at] <= done]
        assert ready
        if how == "shuffle":
            op = ready[int(rng.integers(len(ready)))]
        else:
            op = (min if how == "ascending" else max)(ready, key=lambda o: (o.size, -o.at if how == "descending" else o.at))
        out.append(op)
        done.add(op.at)
        left.remove(op)
    return out


def extent(op):
    """(H, W) of an op on planes, (H, W, D) of one on volumes."""
    return tuple(op.shape) + ((op.depth,) if hasattr(op, "depth") else ())


def check_order(order, seq):
    """What every order must keep: each op after the ops it names; between a multi-scale forward and its backward the forwards that
    overwrite the pyramid (the same entry on other pairs of the same shape and count, the same entry at another shape, another
    multi-scale entry -- of the forward's shape and count where it has the forward's dimensions); the twins first and last."""
    pos = dict((op.at, i) for i, op in enumerate(order))
    for op in order:
        for a in op.after:
            if a.at in pos:
                assert pos[a.at] < pos[op.at], (a.name, op.name)
        for b in getattr(op, "between", ()):
            if op.of.at in pos:
                assert pos[op.of.at] < pos[b.at] < pos[op.at], (op.of.name, b.name, op.name)
                assert b.entry.startswith("enqueue_msssim") and b.pairs is not op.of.pairs
    if len(order) == len(seq.ops):
        assert order[0] is seq.twins[0] and order[-1] is seq.twins[1]
        assert len([op for op in order if op.entry != "enqueue_batch"]) >= 2 * 8 + 1
        for op in order:
            if hasattr(op, "between"):
                f, (s, d, o) = op.of, op.between
                assert (s.entry, extent(s), s.n, s.config) == (f.entry, extent(f), f.n, f.config) and (d.entry, d.config) == (f.entry, f.config)
                assert extent(d) != extent(f) and o.entry != f.entry
                assert (extent(o), o.n) == (extent(f), f.n) or len(extent(o)) != len(extent(f))


def show(title, order):
    print("\n%s: %d ops" % (title, len(order)))
    for i, op in enumerate(order):
        print("  %2d  %s" % (i, op.describe()))


def issue_all(ctx, order, trims=()):
    """The ops of `order` on one context, no synchronise between them (trims: trim() before the ops at these positions); one synchronise."""
    for i, op in enumerate(order):
        if i in trims:
            ctx.trim()
        op.issue(ctx)
    _sync(ctx)


def assert_same_bytes(seq, lone, what):
    """Every byte of every output of every op against the lone call's; every output that differs is named, the first in detail."""
    bad = []
    for op in seq.ops:
        for o in op.outs:
            got = o.read()
            if got.tobytes() == lone[op.name][o.name]:
                continue
            want = np.frombuffer(lone[op.name][o.name], o.init.dtype).reshape(o.init.shape)
            at = np.flatnonzero(got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))
            stray = int(np.count_nonzero((got != o.init) & ~o.owned))
            bad.append("%s of %s: %d of %d bytes differ from the op issued alone, the first at byte %d; %d sentinel elements changed\n      %s" % (
                o.name, op.name, len(at), got.nbytes, at[0], stray, op.describe()))
    assert not bad, "%s: %d outputs differ\n  %s" % (what, len(bad), "\n  ".join(bad))


# ---- the module's fixtures ----------------------------------------------------------------------------------------------------------------

class Meter(object):
    def __init__(self, ctx, what="mixed step"):
        self.ctx, self.t0, self.what = ctx, time.time(), what
        self.free0 = self.min_free = ssim_amd.memory_info(ctx)[0]

    def sample(self):
        self.min_free = min(self.min_free, ssim_amd.memory_info(self.ctx)[0])

    def close(self):
        print("\n%s: module wall time %.1f s; peak device memory in use by the module %.1f MiB" % (
            self.what, time.time() - self.t0, (self.free0 - self.min_free) / 2.0 ** 20))


@pytest.fixture(scope="module")
def meter(gpu_ctx):
    m = Meter(gpu_ctx)
    yield m
    m.close()


def lone_results(seq, meter, hold):
    """{op name: {output name: bytes}} of every op of `seq` issued ALONE on a context created for that purpose, synchronised after every
    op and closed at the end; `seq` is freed.  What the lone results themselves fail -- a sentinel changed, a model missed (hold(ctx, seq,
    results)) -- is kept under "" for test_lone_results_keep_their_sentinels_and_meet_the_models; the other tests compare with these bytes
    either way."""
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    ctx = ssim_amd.Context(0)
    try:
        out = {}
        for op in seq.ops:                                       # list order keeps every backward after its forward
            op.issue(ctx)
            _sync(ctx)
            out[op.name] = op.read()
        meter.sample()
        try:
            for op in seq.ops:
                for o in op.outs:
                    got = np.frombuffer(out[op.name][o.name], o.init.dtype).reshape(o.init.shape)
                    assert np.array_equal(got[~o.owned], o.init[~o.owned]), (op.name, o.name, "a sentinel changed")
                    # (a 16-bit gradient may equal the 16-bit sentinel by coincidence: 203.25 in float16)
                    assert np.count_nonzero(got[o.owned] == o.init[o.owned]) <= (2 if o.init.itemsize == 2 else 0), (op.name, o.name, "elements the op owns were not written")
            hold(ctx, seq, out)
            out[""] = None
        except (AssertionError, ssim_amd.SsimError):
            out[""] = traceback.format_exc()
    finally:
        ctx.close()
        seq.free()
    return out


@pytest.fixture(scope="module")
def lone(gpu_ctx, manifest, meter):
    """lone_results of the sequence: computed once and shared."""
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    return lone_results(Sequence(gpu_ctx, manifest), meter, hold_to_the_models)


@pytest.fixture
def seq(gpu_ctx, manifest, lone, meter):
    s = Sequence(gpu_ctx, manifest)
    yield s
    meter.sample()
    s.free()


# ---- the lone results against the float64 models --------------------------------------------------------------------------------------

def _outs(seq, lone, name):
    """{output name: array} of one op's lone result, planes and vectors extracted."""
    op, res = seq.by_name[name], {}
    for o in op.outs:
        host = np.frombuffer(lone[name][o.name], o.init.dtype).reshape(o.init.shape)
        res[o.name] = o.plane(host) if isinstance(o, (PlaneOut, VolOut)) else o.vec(host)
    return op, res


def _rel(g, want):
    return float(np.abs(g.astype(np.float64) - want).max() / np.abs(want).max())


def _alone(ctx, seq, build):
    """Ops that are no part of the sequence (the float32 twins of the 16-bit ops), added by build(), each issued alone:
    [{output name: array}] per op; removed and freed afterwards."""
    n0 = len(seq.ops)
    try:
        build()
        res = []
        for op in seq.ops[n0:]:
            op.issue(ctx)
            _sync(ctx)
            res.append(dict((o.name, o.plane(o.read()) if isinstance(o, (PlaneOut, VolOut)) else o.vec(o.read())) for o in op.outs))
        return res
    finally:
        for op in seq.ops[n0:]:
            del seq.by_name[op.name]
            for x in op.outs + op.keep:
                x.free()
        del seq.ops[n0:]


def hold_to_the_models(ctx, seq, lone):
    """Pair 0 of one op per entry against its float64 model at the bounds of the family's own module; prints every figure first."""
    px = lambda shape: float(shape[0]) * float(shape[1])
    # ssim16
    op, r = _outs(seq, lone, "ssim16.twocol")
    a, b = op.pairs[0]
    gv, gm = M16.ssim(a.astype(np.int64), b.astype(np.int64), 10)
    e_px, e_g = float(np.abs(r["map0"].astype(np.float64) - gm).max()), abs(float(np.float32(r["sums"][0] / px(op.shape))) - gv)
    print("ssim16.twocol alone: per pixel %.3g (bound %.3g), global %.3g (bound %.3g)" % (e_px, PX16_TOL, e_g, G16_TOL))
    assert e_px <= PX16_TOL and e_g <= G16_TOL
    # ssimf and the windows: value, map, gradient, map gradient
    for fname, gname, mname, window in (("ssimf.gold", "ssimf.gold.g", None, None), ("ssimf.small", "ssimf.small.g", "ssimf.small.m", None),
                                        ("ssimf.twocol", None, "ssimf.twocol.m", None),
                                        ("win7u.twocol", "win7u.twocol.g", None, WIN7U), ("win7u.small", None, "win7u.small.m", WIN7U),
                                        ("win5g.gold", None, "win5g.gold.m", WIN5G), ("win5g.twocol", "win5g.twocol.g", None, WIN5G)):
        op, r = _outs(seq, lone, fname)
        a, b = op.pairs[0]
        if window is None:
            (gv, gm), (px_tol, g_tol, grad_tol, map_tol) = MF.ssim(a, b, RANGE), (MF.PX_TOL, MF.G_TOL, MF.GRAD_TOL, MW.WGRAD_TOL)
        else:
            (gv, gm), (px_tol, g_tol, grad_tol, _) = K.ssim(a, b, RANGE, window), K.tolerances(window)
            map_tol = grad_tol
        e_px, e_g = float(np.abs(r["map0"].astype(np.float64) - gm).max()), abs(float(r["sums"][0]) / px(op.shape) - gv)
        print("%s alone: per pixel %.3g (bound %.3g), global %.3g (bound %.3g)" % (fname, e_px, px_tol, e_g, g_tol))
        assert np.all(np.isfinite(r["map0"])) and e_px <= px_tol and e_g <= g_tol, fname
        for name, tol in ((gname, grad_tol), (mname, map_tol)):
            if name is None:
                continue
            g, rg = _outs(seq, lone, name)
            if g.form == "scalar":
                want = MF.grad(a, b, RANGE, float(g.up[0])) if window is None else K.grad(a, b, RANGE, float(g.up[0]), window)
            else:
                want = MW.grad_map(a, b, RANGE, g.up[0]) if window is None else K.grad_map(a, b, RANGE, g.up[0], window)
            for k in range(2):
                if g.which & (1 << k):
                    e = _rel(rg["d%s0" % "AB"[k]], want[k])
                    print("%s alone, d%s: %.3g of max|grad| (bound %.3g)" % (name, "AB"[k], e, tol))
                    assert e <= tol, (name, k, e)
    # msssimf: value, means, gradient
    for fname in ("msf.twocol", "msf.gold"):
        op, r = _outs(seq, lone, fname)
        g, rg = _outs(seq, lone, fname + ".grad")
        scales, weights = op.config
        mod = MS.Model(op.pairs[0][0], op.pairs[0][1], RANGE)
        mv, mm = mod.msssim(scales, weights)
        e_v, e_m = abs(float(r["values"][0]) - mv), float(np.abs(r["means"][:2 * scales].reshape(scales, 2) - mm).max())
        print("%s alone: value %.3g (bound %.3g), per-scale means %.3g (bound %.3g)" % (fname, e_v, MS.VALUE_TOL, e_m, MS.MEAN_TOL))
        assert e_v <= MS.VALUE_TOL and e_m <= MS.MEAN_TOL, fname
        want = mod.grad(float(g.up[0]), scales, weights)
        for k in range(2):
            if g.which & (1 << k):
                e = _rel(rg["d%s0" % "AB"[k]], want[k])
                print("%s.grad alone, d%s: %.3g of max|grad| (bound %.3g)" % (fname, "AB"[k], e, MS.GRAD_TOL))
                assert e <= MS.GRAD_TOL, (fname, k, e)
    # the 16-bit encodings: the bits of the float32 entries on the widened planes (held to the model above and here), the gradients
    # rounded once
    for fname, gname, form in (("ssimh.f16.twocol", "ssimh.f16.twocol.g", "scalar"), ("ssimh.bf16.small", "ssimh.bf16.small.g", "scalar"),
                               ("ssimh.f16.small", "ssimh.f16.small.m", "map"), ("ssimh.bf16.gold", "ssimh.bf16.gold.m", "map")):
        op, r = _outs(seq, lone, fname)
        g, rg = _outs(seq, lone, gname)
        enc = op.kw["enc"]
        wide = [(HM.widen(a, enc), HM.widen(b, enc)) for a, b in op.pairs]
        def twins():
            wf = seq.forward("widened", "f", wide)
            seq.backward("widened.g", wf, form, which=g.which, salt=g.salt, g_out=g.up if form == "scalar" else None)
        w, wg = _alone(ctx, seq, twins)
        assert r["sums"].tobytes() == w["sums"].tobytes() and all(HM.same_f32(r["map%d" % i], w["map%d" % i]) for i in range(op.n)), fname
        gv, gm = MF.ssim(wide[0][0], wide[0][1], RANGE)
        e_px, e_g = float(np.abs(w["map0"].astype(np.float64) - gm).max()), abs(float(w["sums"][0]) / px(op.shape) - gv)
        print("%s alone: the bits of ssimf on the widened planes; those: per pixel %.3g (bound %.3g), global %.3g (bound %.3g)" % (fname, e_px, MF.PX_TOL, e_g, MF.G_TOL))
        assert e_px <= MF.PX_TOL and e_g <= MF.G_TOL, fname
        for key in rg:
            assert HM.same(rg[key], HM.round_to(wg[key], enc), enc) and (rg[key] & 0x7FFF).max() > 0, (gname, key)
        print("%s alone: the bits of the float32 gradient on the widened planes, rounded once" % gname)
    for fname in ("msh.f16.twocol", "msh.bf16.small"):
        op, r = _outs(seq, lone, fname)
        g, rg = _outs(seq, lone, fname + ".grad")
        scales, weights = op.config
        wide = [(HM.widen(a, op.enc), HM.widen(b, op.enc)) for a, b in op.pairs]
        def twins():
            wf = seq.ms_forward("widened", wide, op.config)
            seq.ms_backward("widened.grad", wf, g.which, [], g_out=g.up)
        w, wg = _alone(ctx, seq, twins)
        assert r["values"].tobytes() == w["values"].tobytes() and r["means"].tobytes() == w["means"].tobytes(), fname
        mod = MS.Model(wide[0][0], wide[0][1], RANGE)
        mv, mm = mod.msssim(scales, weights)
        e_v, e_m = abs(float(r["values"][0]) - mv), float(np.abs(r["means"][:2 * scales].reshape(scales, 2) - mm).max())
        print("%s alone: the bits of msssimf on the widened planes; value %.3g (bound %.3g), per-scale means %.3g (bound %.3g)" % (fname, e_v, MS.VALUE_TOL, e_m, MS.MEAN_TOL))
        assert e_v <= MS.VALUE_TOL and e_m <= MS.MEAN_TOL, fname
        for key in rg:
            assert HM.same(rg[key], HM.round_to(wg[key], op.enc), op.enc) and (rg[key] & 0x7FFF).max() > 0, (fname, key)
        print("%s.grad alone: the bits of the float32 gradient on the widened planes, rounded once" % fname)
    # the volumes: value, map and gradients of one pair per op against the float64 model (tests/ssim3f_model.py)
    px_tol, g_tol, grad_tol, _ = S3.tolerances()
    for fname, i in (("vol.small", 2), ("vol.one", 0), ("vol.big", 1)):
        op, r = _outs(seq, lone, fname)
        g, rg = _outs(seq, lone, fname + ".g")
        a, b = op.pairs[i]
        gv, gm = S3.ssim(a, b, RANGE)
        e_px, e_g = float(np.abs(r["map%d" % i].astype(np.float64) - gm).max()), abs(float(r["sums"][i]) / S3.voxels(a.shape) - gv)
        print("%s alone, pair %d: per voxel %.3g (bound %.3g), global %.3g (bound %.3g)" % (fname, i, e_px, px_tol, e_g, g_tol))
        assert np.all(np.isfinite(r["map%d" % i])) and e_px <= px_tol and e_g <= g_tol, fname
        want = S3.grad(a, b, RANGE, float(g.up[i]))
        for k in range(2):
            if g.which & (1 << k):
                e = _rel(rg["d%s%d" % ("AB"[k], i)], want[k])
                print("%s.g alone, pair %d, d%s: %.3g of max|grad| (bound %.3g)" % (fname, i, "AB"[k], e, grad_tol))
                assert e <= grad_tol, (fname, k, e)
    # the uint8 batch: the committed golden values
    op, r = _outs(seq, lone, "batch8")
    for i, name in enumerate(GOLDEN):
        ent = seq.manifest[name]
        got = "0x%08x" % ssim_amd.finalize(r["sums"][i:i + 1], ent["width"], ent["height"]).view(np.uint32)[0]
        assert got == ent["fma"]["ssim_hex"], (name, got, ent["fma"]["ssim_hex"])


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------

def test_lone_results_keep_their_sentinels_and_meet_the_models(lone):
    assert lone[""] is None, lone[""]


@pytest.mark.parametrize("how", ["ascending", "descending", "shuffle"])
def test_every_output_of_the_mixed_step_has_the_bytes_of_the_call_alone(seq, lone, how):
    order = order_of(seq.ops, how, twins=seq.twins)
    check_order(order, seq)
    show("mixed step, %s" % how, order)
    if how != "shuffle":
        sizes = [op.size for op in order]
        assert sum(1 for x, y in zip(sizes, sizes[1:]) if (y < x if how == "ascending" else y > x)) <= len(sizes) // 3      # only where a dependency demands it
    with ssim_amd.Context(0) as ctx:
        issue_all(ctx, order)
        assert_same_bytes(seq, lone, how)
        first, last = (dict((o.name, o.read().tobytes()) for o in t.outs) for t in seq.twins)
        assert first == last, "the same op on the same pairs, first and last in the sequence"


def test_trims_in_the_middle_and_a_trimmed_context_change_no_byte(seq, lone, manifest, gpu_ctx):
    order = order_of(seq.ops, "ascending", twins=seq.twins, phases=True)      # forwards, then backwards: both ascending
    check_order(order, seq)
    third = len(order) // 3
    trims = (third, 2 * third)
    after = [op.name for i, op in enumerate(order) if hasattr(op, "of") and any(order.index(op.of) < t <= i for t in trims)]
    show("mixed step, ascending, trim() before ops %d and %d" % trims, order)
    print("backwards whose forward ran before a trim that they come after: %s" % " ".join(after))
    assert len(after) == len([op for op in order if hasattr(op, "of")]) and sum(n.endswith(".grad") for n in after) == 5
    with ssim_amd.Context(0) as ctx:
        issue_all(ctx, order, trims)
        assert_same_bytes(seq, lone, "with trims")
        assert ctx.lib.rmgr_ssim_hip_trim(ctx.handle) == 0
        again = Sequence(gpu_ctx, manifest)                      # fresh sentinels: what the second pass leaves is its own
        try:
            issue_all(ctx, order_of(again.ops, "ascending", twins=again.twins, phases=True))
            assert_same_bytes(again, lone, "after a trim, on the empty context")
        finally:
            again.free()


def test_two_contexts_on_two_streams_alternately(seq, lone):
    """No launcher and no host flow keeps mutable state outside its context."""
    halves, group, roots = ([], []), {}, 0                       # ops tied by `after` share a half
    for op in seq.ops:
        tied = set(group[a.at] for a in op.after)
        assert len(tied) <= 1, op.name
        if tied:
            group[op.at] = tied.pop()
        else:
            group[op.at], roots = roots % 2, roots + 1
        halves[group[op.at]].append(op)
    orders = [order_of(h, "shuffle", SHUFFLE_SEED + i) for i, h in enumerate(halves)]
    for i, o in enumerate(orders):
        check_order(o, seq)
        show("two contexts, context %d" % i, o)
    assert min(len(o) for o in orders) >= 17
    with ssim_amd.Context(0) as c0, ssim_amd.Context(0) as c1:
        for i in range(max(len(o) for o in orders)):
            for ctx, o in ((c0, orders[0]), (c1, orders[1])):
                if i < len(o):
                    o[i].issue(ctx)
        _sync(c0)
        _sync(c1)
        assert_same_bytes(seq, lone, "two contexts")


# ---- torch -----------------------------------------------------------------------------------------------------------------------------------
# torch brings a HIP runtime of its own, which has to be the first one a process loads: the checks run in one child process
# (tests/tools/mixed_step_torch_checks.py) that imports torch before the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    tool = os.path.join(ROOT, "tests", "tools", "mixed_step_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "mixed_step_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["combined_step_has_the_bits_of_each_loss_alone", "steps_of_changing_shape", "two_streams"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
