"""GPU: the VOLUME entries inside one training step's mix of calls on ONE context, held to each call alone.

Why.  tests/test_gpu_mixed_step.py drives one context the way a training step does, but of the volume family it knows only enqueue_ssim3f
and enqueue_ssim3f_grad.  The entries merged since -- ssim3f under a window, the map gradient with and without a window, ssim3h in both
encodings with and without a window, msssim3f -- take their descriptor tables from the same ring of 8 slots, their cell partials from the
same buffer and their coefficient volumes from ONE scratch (s3_coef), and msssim3f rebuilds its pyramid, its coarse gradient volumes and
its k_s in the buffers the 2-D multi-scale families rebuild on every call: a 2-D forward and a 3-D backward meet in the same allocation.
All of them are instantiations of one walk and one adjoint (ssim3_walk.h), so a host flow that sizes or offsets the shared scratch wrongly
for one of them corrupts a NEIGHBOUR in the queue.  That is what a comparison with the op issued alone sees and what a per-family test with a
synchronise after every call cannot.

What is asserted.  As in test_gpu_mixed_step (whose Sequence, orders and byte comparison this module imports): 40 enqueues go onto one
context back to back without a host wait, one synchronise and one read-back follow, and every byte of every output buffer -- fp64 sums,
maps, values, per-scale means, float32 and 16-bit gradient volumes, the sentinels between the samples of step-2 volumes and around every
fp64 vector -- equals the byte the same op leaves when it is issued ALONE on a second context that is synchronised after every op.  No
tolerance.  So that "the same wrong bits on both sides" is excluded, pair 0 of every volume op's lone result is held to its float64 model
at the bound the family's own module asserts: ssim3f_model.tolerances(), ssim3w_model.tolerances(), ssim3k_model.tolerances(window),
msssim3f_model.tolerances() (after asserting m_s >= 0.2 for every weighted scale of the very pairs held); the 16-bit entries by the
header's contract: sums and maps have the bits of the float32 entry on the widened volumes, gradients are that entry's float32 gradient
rounded once, and the widened float32 twin is held to the float64 model.  No bound is new.

The sequence (Sequence3.build).  Sizes are W x H x D: 33 x 20 x 13 (three tiles in x, two in y, an 8-slice cell and a 5-slice one),
65 x 63 x 40 (one voxel past four tiles in x, five cells; its pyramid goes 33 x 32 x 20, 17 x 16 x 10, 9 x 8 x 5, 5 x 4 x 3) and
5 x 3 x 40 (both lateral axes shorter than every window, five cells).  ssim3f under the 7-tap box and the 5-tap Gaussian of sigma 0.8 with
maps and scalar gradients; the map gradient from seeded standard-normal upstream volumes (one of them two floats apart) under the fixed
window and under the Gaussian; ssim3h in float16 and bfloat16, with and without a window, with scalar and map gradients into uint16
volumes; msssim3f at Wang's five scales and at three scales of its own weights, each forward F followed, BEFORE its backward, by msssim3f
of other pairs of F's shape and count, msssim3f of one pair of the other shape and a 2-D multi-scale forward (msssimf; msssimh in
bfloat16): the backward rebuilds its pyramid in buffers a 2-D call has just refilled and takes its means from F's own buffer.  They
collide with plain ssim3f and its gradient, ssimf of 8 x 512 x 512 (which regrows the cell partials beyond any volume op here), an
msssimf group of 4 x 512 x 512, a windowed 2-D ssimf with its gradient, and ssimf of one 33 x 17 pair first and last.

Conditions on the sequence, asserted from the plain-Python planners whenever a Sequence3 is built (conditions();
tests/test_mixed_step3_cpu.py builds one without a device): at least 2 x 8 + 1 ring ops; at least 10 distinct volume entry points; a 2-D
multi-scale op needs more msf_pyramid floats than every msssim3f op and an msssim3f op more than some 2-D one; the s3_coef needs of the
volume backwards take at least four values and the two largest belong to different families.  On the orders themselves (pyramid_walk()):
the ascending order regrows msf_pyramid across the 2-D / 3-D boundary; in the descending order the buffers, which only grow, are sized by
the 2-D op of 4 x 512 x 512 that comes first, so nothing can regrow them: what is asserted there is that an msssim3f backward runs in a
pyramid a 2-D op sized (its own 2-D forward having refilled it in between, which check_order asserts).

Orders and tests: as test_gpu_mixed_step's -- ascending, descending and a seeded shuffle; every forward then every backward with trim()
before each third (every backward follows a trim that its forward preceded) and once more on the trimmed context; two dependency-closed
halves on two contexts alternately; the torch half (tests/tools/mixed_step3_torch_checks.py) in one child process.

After a return code that is neither success nor EINVAL the module starts nothing more on the GPU (test_gpu_ssimk's _device_error, shared
with that module).  Every test frees its own buffers.  The module prints its wall time and its peak device memory when it ends.

Cost, measured on an MI355X: the 9 tests take 4.0 s together (3.1 s of it the torch child process, 0.9 s the lone calls with their float32
twins and float64 models), no other test more than 0.1 s of its own; the device holds 106 MiB more than before the module at the peak.
On the pairs held, the lone results stay below 1 % of their bounds (the largest: 3.2e-6 of max|grad| against 6.2e-4, the map gradient of
the 5 x 3 x 40 volume).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import halfmodel as HM
import msssim3f_model as M3
import msssim3f_plan as MP
import msssimf_model as MS
import sample_forms_inputs as IN
import ssim3f_model as S3
import ssim3f_plan as P
import ssim3k_model as K3
import ssim3w_model as W3
import ssimk_model as K
import ssim_amd
from conftest import ROOT
from ssim3f_chunks_inputs import SF_SLOTS
from test_gpu_mixed_step import (BIG, MS3, MS5, RANGE, SHUFFLE_SEED, SMALL, TWOCOL, VOL, VOLBIG, WIN5G, WIN7U, Meter, Op, Out, PlaneOut,  # noqa: F401
                                 Sequence, VecOut, VolOut, _alone, _outs, _rel, _sync, assert_same_bytes, check_order, extent, issue_all,
                                 lone_results, order_of, pairs_3f, pairs_f, pairs_h, show)
from test_gpu_ssimk import _device_error, mk
from test_gpu_ssimw import FILL32

pytestmark = pytest.mark.gpu

THIN = (5, 3, 40)                                            # W x H x D: both lateral axes shorter than every window, five cells
F16, BF16 = HM.F16, HM.BF16
MIN_MEAN = 0.2                                               # msssim3f_model's bounds hold where every weighted m_s is at least this


def pairs_3h(size, n, salt, enc):
    """pairs_3f's draws rounded once into the encoding: uint16 bit patterns."""
    return [(HM.round_to(a, enc), HM.round_to(b, enc)) for a, b in pairs_3f(size, n, salt)]


def upstream3(shape, n, salt):
    """n per-voxel upstream gradients: the "normal" volume of ssim3w_model.weight_volumes, one seed per pair."""
    return [next(v for k, v in W3.weight_volumes(shape, seed=salt + i) if k == "normal") for i in range(n)]


class DryMem(object):
    """Stands in for the context that owns a sequence's buffers where only the PLAN of the sequence is wanted: upload() hands out
    addresses that are never used; no device, no library call."""

    class Buf(object):
        def __init__(self, ptr):
            self.ptr = ptr

        def free(self):
            self.ptr = None

    def __init__(self):
        self.next = 1 << 20

    def upload(self, arr):
        b = DryMem.Buf(self.next)
        self.next += (np.asarray(arr).nbytes + 255) // 256 * 256 + 256
        return b


# ---- the sequence ------------------------------------------------------------------------------------------------------------------------

class Sequence3(Sequence):
    """The volume step: Sequence's builders and these for every volume entry."""

    def volume(self, name, pairs, window=None, enc=None, maps=None, step=1, after=()):
        """enqueue_ssim3f / enqueue_ssim3h (enc: uint16 bit patterns) of `pairs` ((D, H, W) arrays, dense in device memory), under
        `window` (None: the fixed one); maps: the pairs that get a float32 map (None: all), `step` floats apart."""
        mem, n, (d, h, w), half = self.mem, len(pairs), pairs[0][0].shape, enc is not None
        assert pairs[0][0].dtype == (np.uint16 if half else np.float32)
        ps = ((ssim_amd.Params3H if half else ssim_amd.Params3F) * n)()
        make = ssim_amd.make_params3h if half else ssim_amd.make_params3f
        keep, outs = [], []
        for i, (a, b) in enumerate(pairs):
            da, db = mem.upload(a), mem.upload(b)
            keep += [da, db]
            m = None
            if maps is None or i in maps:
                m = VolOut(mem, "map%d" % i, d, h, w, step)
                outs.append(m)
            ps[i] = make(w, h, d, da.ptr, (1, w, w * h), db.ptr, (1, w, w * h), m.ptr if m else None, m.strides if m else None)
        sums = VecOut(mem, "sums", n)
        outs.append(sums)
        win = mk(window)
        if half:
            entry, call = "enqueue_ssim3h", lambda ctx: ctx.enqueue_ssim3h(ps, n, RANGE, enc, sums.ptr, window=win)
        else:
            entry, call = "enqueue_ssim3f", lambda ctx: ctx.enqueue_ssim3f(ps, n, RANGE, sums.ptr, window=win)
        entry += "_win" if window else ""
        note = "depth %d, %s%s, %d maps, step %d" % (d, enc + ", " if half else "", K.name_of(window or K.DEFAULT), len(outs) - 1, step)
        op = self.add(Op(name, entry, (h, w), n, note, call, outs, keep, after))
        op.kind, op.enc, op.window, op.params, op.pairs, op.depth, op.maps, op.step = "3h" if half else "3f", enc, window, ps, pairs, d, maps, step
        op.size *= d
        return op

    def volume_grad(self, name, f, form, which=3, step=1, salt=0, ustep=1, g_out=None, after=()):
        """The gradient of the volume forward f's pairs under f's window, in f's encoding: form "scalar" (g_out per pair; default: -0.75
        -- 16-bit: W H D, so that the rounded voxels are normal numbers -- times 1, 1.5, 2 ...) or "map" (a seeded upstream volume per
        pair, its samples `ustep` floats apart)."""
        mem, n, (h, w), d, half = self.mem, f.n, f.shape, f.depth, f.enc is not None
        cls, dt = (ssim_amd.Grad3H, np.uint16) if half else (ssim_amd.Grad3F, np.float32)
        arrs, outs, keep = [None, None], [], []
        for k in range(2):
            if which & (1 << k):
                arrs[k] = (cls * n)()
                for i in range(n):
                    g = VolOut(mem, "d%s%d" % ("AB"[k], i), d, h, w, step, dt)
                    outs.append(g)
                    arrs[k][i] = cls(g.ptr, *g.strides)
        ps, win, enc = f.params, mk(f.window), f.enc
        if form == "scalar":
            if g_out is None:
                g_out = np.float32([(float(w * h * d) if half else IN.G_OUT) * (1.0 + 0.5 * i) for i in range(n)])
            go = mem.upload(g_out)
            keep.append(go)
            if half:
                entry, call = "enqueue_ssim3h", lambda ctx: ctx.enqueue_ssim3h_grad(ps, n, RANGE, enc, go.ptr, arrs[0], arrs[1], window=win)
            else:
                entry, call = "enqueue_ssim3f", lambda ctx: ctx.enqueue_ssim3f_grad(ps, n, RANGE, go.ptr, arrs[0], arrs[1], window=win)
            entry += ("_win" if f.window else "") + "_grad"
            up = g_out
        else:
            up = upstream3((d, h, w), n, salt)
            ms = (ssim_amd.GradOut3F * n)()
            for i in range(n):
                host = np.full((d, h, w, ustep), FILL32, np.float32)
                host[..., ustep - 1] = up[i]
                m = mem.upload(host)
                keep.append(m)
                ms[i] = ssim_amd.GradOut3F(m.ptr + 4 * (ustep - 1), ustep, ustep * w, ustep * w * h)
            if half:
                entry, call = "enqueue_ssim3h", lambda ctx: ctx.enqueue_ssim3h_map_grad(ps, n, RANGE, enc, ms, arrs[0], arrs[1], window=win)
            else:
                entry, call = "enqueue_ssim3f", lambda ctx: ctx.enqueue_ssim3f_map_grad(ps, n, RANGE, ms, arrs[0], arrs[1], window=win)
            entry += ("_win" if f.window else "") + "_map_grad"
        note = "of %s, %s, depth %d, step %d%s" % (f.name, ("dA", "dB", "dA dB")[which - 1], d, step, ", upstream step %d" % ustep if form == "map" else "")
        op = self.add(Op(name, entry, (h, w), n, note, call, outs, keep, [f] + list(after)))
        op.of, op.form, op.which, op.up, op.salt, op.ustep, op.depth, op.enc, op.window = f, form, which, up, salt, ustep, d, enc, f.window
        op.size *= d
        return op

    # -- multi-scale volumes --

    def ms3_forward(self, name, pairs, config, after=()):
        mem, n, (d, h, w) = self.mem, len(pairs), pairs[0][0].shape
        scales, weights = config
        ps = (ssim_amd.Params3F * n)()
        keep = []
        for i, (a, b) in enumerate(pairs):
            da, db = mem.upload(a), mem.upload(b)
            keep += [da, db]
            ps[i] = ssim_amd.make_params3f(w, h, d, da.ptr, (1, w, w * h), db.ptr, (1, w, w * h))
        values, means = VecOut(mem, "values", n), VecOut(mem, "means", n * scales * 2)
        op = self.add(Op(name, "enqueue_msssim3f", (h, w), n, "depth %d, %d scales" % (d, scales),
                         lambda ctx: ctx.enqueue_msssim3f(ps, n, RANGE, values.ptr, means.ptr, scales, weights), [values, means], keep, after))
        op.kind, op.enc, op.window, op.config, op.params, op.pairs, op.means, op.depth = "ms3", None, None, config, ps, pairs, means, d
        op.size *= d
        return op

    def ms3_backward(self, name, f, which, between, step=1, g_out=None):
        """The backward of the multi-scale volume forward f from f's own means buffer, after every forward of `between`."""
        mem, n, (h, w), d = self.mem, f.n, f.shape, f.depth
        ps, (scales, weights), means = f.params, f.config, f.means
        arrs, outs = [None, None], []
        for k in range(2):
            if which & (1 << k):
                arrs[k] = (ssim_amd.Grad3F * n)()
                for i in range(n):
                    g = VolOut(mem, "d%s%d" % ("AB"[k], i), d, h, w, step)
                    outs.append(g)
                    arrs[k][i] = ssim_amd.Grad3F(g.ptr, *g.strides)
        if g_out is None:
            g_out = np.float32([IN.G_OUT * (1.0 + 0.5 * i) for i in range(n)])
        go = mem.upload(g_out)
        note = "of %s, %s, depth %d, step %d, after %s" % (f.name, ("dA", "dB", "dA dB")[which - 1], d, step, " ".join(b.name for b in between))
        op = self.add(Op(name, "enqueue_msssim3f_grad", (h, w), n, note,
                         lambda ctx: ctx.enqueue_msssim3f_grad(ps, n, RANGE, means.ptr, go.ptr, arrs[0], arrs[1], scales, weights),
                         outs, [go], [f] + list(between)))
        op.of, op.which, op.up, op.between, op.depth, op.enc, op.window = f, which, g_out, list(between), d, None, None
        op.size *= d
        return op

    def ms3_group(self, tag, pairs, others, config, which, other_size, plane_pairs, plane_config, plane_enc=None, step=1):
        """A multi-scale volume forward, its backward, and between the two: msssim3f of other pairs of the same shape and count, msssim3f
        of one pair of the other shape, and a 2-D multi-scale forward (msssimf, or msssimh in plane_enc)."""
        f = self.ms3_forward(tag, pairs, config)
        same_shape = self.ms3_forward(tag + ".same", others, config, after=[f])
        at_other_shape = self.ms3_forward(tag + ".shape", pairs_3f(other_size, 1, 900 + len(self.ops)), config, after=[f])
        two_d = self.ms_forward(tag + ".family", plane_pairs, plane_config, plane_enc, after=[f])
        return f, self.ms3_backward(tag + ".grad", f, which, [same_shape, at_other_shape, two_d], step)

    def build(self):
        # the same pairs (the same device planes) twice, first and last, into different outputs
        first = self.forward("ssimf.first", "f", pairs_f(SMALL, 1, 1))
        # ssim3f under a window: forward with maps, scalar gradient; the Gaussian on the large volume also with its map gradient
        u_vol = self.volume("w7u.vol", pairs_3f(VOL, 2, 40), window=WIN7U)
        g_big = self.volume("w5g.big", pairs_3f(VOLBIG, 1, 41), window=WIN5G)
        self.volume_grad("w7u.vol.g", u_vol, "scalar")
        self.volume_grad("w5g.big.g", g_big, "scalar", which=1)
        self.volume_grad("w5g.big.m", g_big, "map", which=2, salt=70)
        # the windowed 2-D family and the largest user of the cell partials
        u_two = self.forward("win7u.twocol", "k", pairs_f(TWOCOL, 2, 7), window=WIN7U)
        self.backward("win7u.twocol.g", u_two, "scalar")
        self.forward("ssimf.big", "f", pairs_f(BIG, 8, 6), maps=(0, 7))
        # ssim3h: both encodings, fixed window: scalar gradient, map gradient
        h_vol = self.volume("h.f16.vol", pairs_3h(VOL, 2, 43, F16), enc=F16)
        b_big = self.volume("h.bf16.big", pairs_3h(VOLBIG, 1, 44, BF16), enc=BF16)
        self.volume_grad("h.f16.vol.g", h_vol, "scalar")
        self.volume_grad("h.bf16.big.m", b_big, "map", salt=80)
        # msssim3f at Wang's five scales on the small volumes; the 2-D forward before its backward is msssimf
        self.ms3_group("ms3.vol", pairs_3f(VOL, 2, 30), pairs_3f(VOL, 2, 32), MS5, 3, VOLBIG, pairs_f(TWOCOL, 2, 47), MS5, step=2)
        # plain ssim3f with maps two floats apart, its gradient, and the map gradient (fixed window) from upstream volumes two floats apart
        v_plain = self.volume("vol.plain", pairs_3f(VOL, 2, 42), step=2)
        self.volume_grad("vol.plain.g", v_plain, "scalar", step=2)
        self.volume_grad("vol.plain.m", v_plain, "map", salt=90, ustep=2)
        # the Gaussian on the small volumes: one gradient
        g_vol = self.volume("w5g.vol", pairs_3f(VOL, 2, 48), window=WIN5G, maps=(1,))
        self.volume_grad("w5g.vol.g", g_vol, "scalar", which=2)
        # the 2-D multi-scale family at 4 x 512 x 512: more pyramid, coarse gradients and k_s than any volume op
        self.ms_group("msf.big", pairs_f(BIG, 4, 16), pairs_f(BIG, 4, 17), MS5, which=3)
        # ssim3h under a window: bfloat16 under the box with its scalar gradient, float16 under the Gaussian on the thin volume with its
        # map gradient
        k_vol = self.volume("hk.bf16.vol", pairs_3h(VOL, 1, 45, BF16), window=WIN7U, enc=BF16)
        k_thin = self.volume("hk.f16.thin", pairs_3h(THIN, 1, 46, F16), window=WIN5G, enc=F16, step=2)
        self.volume_grad("hk.bf16.vol.g", k_vol, "scalar", step=2)
        self.volume_grad("hk.f16.thin.m", k_thin, "map", salt=100)
        # the thin volume: fixed window, map gradient
        v_thin = self.volume("vol.thin", pairs_3f(THIN, 1, 50))
        self.volume_grad("vol.thin.m", v_thin, "map", salt=110)
        # msssim3f at three scales on the large volumes, dA alone; the 2-D forward before its backward is msssimh in bfloat16
        self.ms3_group("ms3.big", pairs_3f(VOLBIG, 2, 31), pairs_3f(VOLBIG, 2, 33), MS3, 1, VOL, pairs_h(SMALL, 2, 49, BF16)[0], MS3, BF16)
        last = self.forward("ssimf.last", "f", pairs_f(SMALL, 1, 1), planes_of=first)
        self.twins = (first, last)
        conditions(self)


# ---- what the planners say about the sequence ---------------------------------------------------------------------------------------------

def is_volume(op):
    return hasattr(op, "depth")


def is_ms(op):
    return op.entry.startswith("enqueue_msssim")


def entry_point(op):
    """The entry an op calls, the window and the encoding counted as part of it."""
    return (op.entry, K.name_of(op.window) if op.window else None, op.enc)


def family(op):
    """The kernel file behind a volume op."""
    if op.entry.startswith("enqueue_msssim3f"):
        return "msssim3f"
    half = op.entry.startswith("enqueue_ssim3h")
    if op.window:
        return "ssim3hk" if half else "ssim3k"
    return "ssim3h" if half else ("ssim3w" if op.entry.endswith("_map_grad") else "ssim3f")


def pyramid_need(op):
    """Floats of msf_pyramid the host flow of a multi-scale op grows the buffer to (both volumes / planes of every pair, scales >= 1):
    msssim3f_plan.pyramid_floats, and msssimf_model.scale_dims for the 2-D families."""
    scales = (op.of if hasattr(op, "of") else op).config[0]
    (h, w), n = op.shape, op.n
    if is_volume(op):
        return 2 * MP.pyramid_floats(w, h, op.depth, scales) * n
    return 2 * sum(ws * hs for ws, hs in MS.scale_dims(w, h, scales)[1:]) * n


def coef_need(op):
    """Bytes of s3_coef the host flow of a volume backward grows the scratch to: ssim3f_plan.grad_scratch per volume; for msssim3f the
    coefficient part of msssim3f_plan.scratch_bytes, which is sized for scale 0 and is the same figure."""
    (h, w), d, n = op.shape, op.depth, op.n
    per = P.grad_scratch(w, h, d, op.which)
    if is_ms(op):
        scales, planes = op.of.config[0], (2 if op.which == 3 else 1)
        assert MP.scratch_bytes(w, h, d, scales, planes) - (2 + planes) * MP.pyramid_floats(w, h, d, scales) * 4 - scales * 4 == per
    return per * n


def conditions(seq, say=False):
    """What the sequence must be for the step to test what it is there for; from the planners, nothing is launched."""
    ring = [op for op in seq.ops if op.entry != "enqueue_batch"]
    points = sorted(set(entry_point(op) for op in ring if is_volume(op)), key=repr)
    assert len(ring) >= 2 * SF_SLOTS + 1, len(ring)
    assert len(points) >= 10, points
    need = [(pyramid_need(op), op) for op in ring if is_ms(op)]
    need3, need2 = [x for x in need if is_volume(x[1])], [x for x in need if not is_volume(x[1])]
    top3, top2, low2 = max(need3, key=lambda x: x[0]), max(need2, key=lambda x: x[0]), min(need2, key=lambda x: x[0])
    assert top2[0] > top3[0], "no 2-D multi-scale op needs more msf_pyramid than every msssim3f op"
    assert top3[0] > low2[0], "no msssim3f op needs more msf_pyramid than some 2-D multi-scale op"
    coef = sorted(((coef_need(op), op) for op in ring if is_volume(op) and hasattr(op, "of")), key=lambda x: -x[0])
    values = sorted(set(c for c, _ in coef), reverse=True)
    assert len(values) >= 4, values
    largest = set(family(op) for c, op in coef if c == values[0])
    second = set(family(op) for c, op in coef if c == values[1])
    assert not (largest & second), (largest, second)
    if say:
        print("\nthe volume step: %d ring ops, %d volume entry points:" % (len(ring), len(points)))
        for p in points:
            print("  %s%s%s" % (p[0], ", " + p[1] if p[1] else "", ", " + p[2] if p[2] else ""))
        print("msf_pyramid: %s needs %d floats, more than every msssim3f op (the most: %s, %d floats); %s needs less than that: %d floats" % (
            top2[1].name, top2[0], top3[1].name, top3[0], low2[1].name, low2[0]))
        print("s3_coef, bytes per volume backward: %s" % ", ".join("%s (%s) %d" % (op.name, family(op), c) for c, op in coef))


def pyramid_walk(order, how):
    """msf_pyramid along an order on a fresh context (the buffer only grows): [(op that regrows it, op that had sized it)] where the two
    differ in dimensions, and [(op, op that sized the pyramid it runs in)] likewise.  Asserted: the ascending order regrows the buffer
    across the 2-D / 3-D boundary; in the descending order an msssim3f op runs in a pyramid a 2-D op sized."""
    floats, by, regrown, guests = 0, None, [], []
    for op in order:
        if not is_ms(op):
            continue
        need = pyramid_need(op)
        if need > floats:
            if by is not None and is_volume(by) != is_volume(op):
                regrown.append((op, by, floats, need))
            floats, by = need, op
        elif is_volume(by) != is_volume(op):
            guests.append((op, by, need, floats))
    for op, was, f0, f1 in regrown:
        print("msf_pyramid, %s: %s regrows it from %d to %d floats after %s had sized it" % (how, op.name, f0, f1, was.name))
    print("msf_pyramid, %s: %d ops run in a pyramid an op of the other dimensions sized, e.g. %s" % (
        how, len(guests), "; ".join("%s (%d floats) in %s's %d" % (op.name, n, was.name, f) for op, was, n, f in guests[:3])))
    if how == "ascending":
        assert regrown, "no regrow of msf_pyramid across the 2-D / 3-D boundary"
    if how == "descending":
        assert any(is_volume(op) and hasattr(op, "of") for op, _, _, _ in guests), "no msssim3f backward in a pyramid a 2-D op sized"
    return regrown, guests


def planned_orders(seq):
    """{title: (order, trims)} of every order the tests issue, each checked (check_order) -- nothing is launched."""
    out = {}
    for how in ("ascending", "descending", "shuffle"):
        order = order_of(seq.ops, how, twins=seq.twins)
        check_order(order, seq)
        if how != "shuffle":
            sizes = [op.size for op in order]
            assert sum(1 for x, y in zip(sizes, sizes[1:]) if (y < x if how == "ascending" else y > x)) <= len(sizes) // 3      # only where a dependency demands it
        out[how] = (order, ())
    order = order_of(seq.ops, "ascending", twins=seq.twins, phases=True)      # forwards, then backwards: both ascending
    check_order(order, seq)
    third = len(order) // 3
    trims = (third, 2 * third)
    backs = [op for op in order if hasattr(op, "of")]
    after = [op.name for i, op in enumerate(order) if hasattr(op, "of") and any(order.index(op.of) < t <= i for t in trims)]
    assert len(after) == len(backs) and sum(is_ms(op) and is_volume(op) for op in backs) == 2, (after, [op.name for op in backs])
    out["trims"] = (order, trims)
    halves, group, roots = ([], []), {}, 0                       # ops tied by `after` share a half
    for op in seq.ops:
        tied = set(group[a.at] for a in op.after)
        assert len(tied) <= 1, op.name
        if tied:
            group[op.at] = tied.pop()
        else:
            group[op.at], roots = roots % 2, roots + 1
        halves[group[op.at]].append(op)
    for i, h in enumerate(halves):
        o = order_of(h, "shuffle", SHUFFLE_SEED + i)
        check_order(o, seq)
        assert len(o) >= 2 * SF_SLOTS + 1 and any(op.entry == "enqueue_msssim3f_grad" for op in o), (i, len(o))
        out["context %d" % i] = (o, ())
    return out


# ---- the module's fixtures ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def meter(gpu_ctx):
    m = Meter(gpu_ctx, "mixed volume step")
    yield m
    m.close()


@pytest.fixture(scope="module")
def lone(gpu_ctx, meter):
    """test_gpu_mixed_step.lone_results of the volume step: computed once and shared."""
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    seq = Sequence3(gpu_ctx, None)
    conditions(seq, say=True)
    return lone_results(seq, meter, hold_to_the_models)


@pytest.fixture
def seq(gpu_ctx, lone, meter):
    s = Sequence3(gpu_ctx, None)
    yield s
    meter.sample()
    s.free()


# ---- the lone results against the float64 models --------------------------------------------------------------------------------------

def models(window):
    """(ssim, grad, grad_map, (PX_TOL, G_TOL, GRAD_TOL, MAPGRAD_TOL)) of the float32 volume entries under a window (None: the fixed one)."""
    if window is None:
        px, g, grad, _ = S3.tolerances()
        return S3.ssim, S3.grad, W3.grad_map, (px, g, grad, W3.tolerances())
    px, g, grad, _, mapgrad = K3.tolerances(window)
    return (lambda a, b, r: K3.ssim(a, b, r, window), lambda a, b, r, go: K3.grad(a, b, r, go, window),
            lambda a, b, r, m: K3.grad_map(a, b, r, m, window), (px, g, grad, mapgrad))


def hold_float32(what, pair, window, res, backs):
    """Pair 0 of a float32 volume forward (res: its outputs) and of its backwards ([(name, op, outputs)]) against the float64 model."""
    ssim, grad, grad_map, (px_tol, g_tol, grad_tol, map_tol) = models(window)
    a, b = pair
    gv, gm = ssim(a, b, RANGE)
    e_g = abs(float(res["sums"][0]) / S3.voxels(a.shape) - gv)
    if "map0" in res:
        e_px = float(np.abs(res["map0"].astype(np.float64) - gm).max())
        print("%s alone: per voxel %.3g (bound %.3g), global %.3g (bound %.3g)" % (what, e_px, px_tol, e_g, g_tol))
        assert np.all(np.isfinite(res["map0"])) and e_px <= px_tol, what
    else:
        print("%s alone: global %.3g (bound %.3g)" % (what, e_g, g_tol))
    assert e_g <= g_tol, what
    for name, g, rg in backs:
        want, tol = (grad(a, b, RANGE, float(g.up[0])), grad_tol) if g.form == "scalar" else (grad_map(a, b, RANGE, g.up[0]), map_tol)
        for k in range(2):
            if g.which & (1 << k):
                e = _rel(rg["d%s0" % "AB"[k]], want[k])
                print("%s alone, d%s: %.3g of max|grad| (bound %.3g)" % (name, "AB"[k], e, tol))
                assert e <= tol, (name, k, e)


def hold_to_the_models(ctx, seq, lone):
    """Pair 0 of every volume op against its float64 model at the bounds of the family's own module; prints every figure first."""
    # ssim3f: the fixed window and the two windows; value, map, gradient, map gradient
    for fname, gnames in (("vol.plain", ("vol.plain.g", "vol.plain.m")), ("vol.thin", ("vol.thin.m",)), ("w7u.vol", ("w7u.vol.g",)),
                          ("w5g.big", ("w5g.big.g", "w5g.big.m"))):
        op, r = _outs(seq, lone, fname)
        hold_float32(fname, op.pairs[0], op.window, r, [(g,) + _outs(seq, lone, g) for g in gnames])
    # (w5g.vol has a map for pair 1 only: its value and its gradient)
    op, r = _outs(seq, lone, "w5g.vol")
    hold_float32("w5g.vol", op.pairs[0], op.window, r, [("w5g.vol.g",) + _outs(seq, lone, "w5g.vol.g")])
    # msssim3f: value, every per-scale mean, the gradients
    value_tol, mean_tol, grad_tol, _ = M3.tolerances()
    for fname in ("ms3.vol", "ms3.big"):
        op, r = _outs(seq, lone, fname)
        g, rg = _outs(seq, lone, fname + ".grad")
        scales, weights = op.config
        wts = MS.check_weights(scales, weights)
        mod = M3.Model(op.pairs[0][0], op.pairs[0][1], RANGE)
        mv, mm = mod.msssim(scales, weights)
        low = min(float(mm[s][1] if s == scales - 1 else mm[s][0]) for s in range(scales) if wts[s] > 0)      # the bounds' input condition
        print("%s, pair 0: lowest weighted m_s %.3f in float64 (the bounds hold from %.1f)" % (fname, low, MIN_MEAN))
        assert low >= MIN_MEAN, (fname, low)
        e_v, e_m = abs(float(r["values"][0]) - mv), float(np.abs(r["means"][:2 * scales].reshape(scales, 2) - mm).max())
        print("%s alone: value %.3g (bound %.3g), per-scale means %.3g (bound %.3g)" % (fname, e_v, value_tol, e_m, mean_tol))
        assert e_v <= value_tol and e_m <= mean_tol, fname
        want = mod.grad(float(g.up[0]), scales, weights)
        for k in range(2):
            if g.which & (1 << k):
                e = _rel(rg["d%s0" % "AB"[k]], want[k])
                print("%s.grad alone, d%s: %.3g of max|grad| (bound %.3g)" % (fname, "AB"[k], e, grad_tol))
                assert e <= grad_tol, (fname, k, e)
    # ssim3h, plain and windowed: the bits of the float32 entries on the widened volumes, the gradients rounded once; those float32
    # twins against the float64 model
    for fname, gname in (("h.f16.vol", "h.f16.vol.g"), ("h.bf16.big", "h.bf16.big.m"), ("hk.bf16.vol", "hk.bf16.vol.g"), ("hk.f16.thin", "hk.f16.thin.m")):
        op, r = _outs(seq, lone, fname)
        g, rg = _outs(seq, lone, gname)
        enc = op.enc
        wide = [(HM.widen(a, enc), HM.widen(b, enc)) for a, b in op.pairs]

        def twins():
            wf = seq.volume("widened", wide, window=op.window, maps=op.maps, step=op.step)
            seq.volume_grad("widened.g", wf, g.form, which=g.which, salt=g.salt, ustep=g.ustep, g_out=g.up if g.form == "scalar" else None)
        w, wg = _alone(ctx, seq, twins)
        assert r["sums"].tobytes() == w["sums"].tobytes() and all(HM.same_f32(r["map%d" % i], w["map%d" % i]) for i in range(op.n)), fname
        assert sorted(rg) == sorted(wg), gname
        for key in rg:
            assert rg[key].dtype == np.uint16 and HM.same(rg[key], HM.round_to(wg[key], enc), enc) and (rg[key] & 0x7FFF).max() > 0, (gname, key)
        print("%s, %s alone: the bits of the float32 entries on the widened volumes, the gradient rounded once; those:" % (fname, gname))
        hold_float32("  float32 twin of %s" % fname, wide[0], op.window, w, [("  float32 twin of %s" % gname, g, wg)])


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------

def test_lone_results_keep_their_sentinels_and_meet_the_models(lone):
    assert lone[""] is None, lone[""]


@pytest.mark.parametrize("how", ["ascending", "descending", "shuffle"])
def test_every_output_of_the_volume_step_has_the_bytes_of_the_call_alone(seq, lone, how):
    order, _ = planned_orders(seq)[how]
    show("volume step, %s" % how, order)
    pyramid_walk(order, how)
    with ssim_amd.Context(0) as ctx:
        issue_all(ctx, order)
        assert_same_bytes(seq, lone, how)
        first, last = (dict((o.name, o.read().tobytes()) for o in t.outs) for t in seq.twins)
        assert first == last, "the same op on the same pairs, first and last in the sequence"


def test_trims_in_the_middle_and_a_trimmed_context_change_no_byte(seq, lone, gpu_ctx):
    order, trims = planned_orders(seq)["trims"]                  # asserts: every backward follows a trim that its forward preceded
    show("volume step, forwards then backwards, ascending, trim() before ops %d and %d" % trims, order)
    with ssim_amd.Context(0) as ctx:
        issue_all(ctx, order, trims)
        assert_same_bytes(seq, lone, "with trims")
        assert ctx.lib.rmgr_ssim_hip_trim(ctx.handle) == 0
        again = Sequence3(gpu_ctx, None)                         # fresh sentinels: what the second pass leaves is its own
        try:
            issue_all(ctx, order_of(again.ops, "ascending", twins=again.twins, phases=True))
            assert_same_bytes(again, lone, "after a trim, on the empty context")
        finally:
            again.free()


def test_two_contexts_on_two_streams_alternately(seq, lone):
    """No launcher and no host flow keeps mutable state outside its context."""
    orders = [planned_orders(seq)["context %d" % i][0] for i in range(2)]
    for i, o in enumerate(orders):
        show("two contexts, context %d" % i, o)
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
# (tests/tools/mixed_step3_torch_checks.py) that imports torch before the library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    tool = os.path.join(ROOT, "tests", "tools", "mixed_step3_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "mixed_step3_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["combined_step_has_the_bits_of_each_loss_alone", "steps_of_changing_shape", "two_streams"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
