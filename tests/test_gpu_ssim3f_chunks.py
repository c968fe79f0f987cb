"""GPU: the scheduling of the volume family (ssim3f: walk, reduction and adjoint kernels, the host flow of ssim_volumes_abi.cpp) -- every chunk
depth plan3f can choose, the sub-batches of a call beyond the launch limit and the descriptor ring beyond its slots: every volume must
have, bit for bit, the sum, the map and the gradients it has when it is launched alone.  Sizes are W x H x D; arrays are (D, H, W).

Why.  plan3f cuts z into chunks of 8, 16, 32, ... slices, by the launch's volume count and the device's CU count alone; a workgroup walks
one chunk, zeroes its fp64 column sum after every 8-slice reduction cell and flushes the cell to its absolute place; the walks of the
backward write and read the coefficient scratch per volume.  "Results do not depend on it" (ssim3f_kernels.h), yet the other modules reach
depth 16 and 32 only by accident of two shapes and no deeper chunk at all.  Chunk depth is scheduling only -- cells sit at absolute
positions, every voxel receives its 11 slices in source order -- so a launch of many volumes, which makes the planner choose deep chunks,
must reproduce the one-volume launch (depth 8, asserted), and the one-volume launch is held to the float64 model at
ssim3f_model.tolerances().  No bound is new.

Shapes (tests/ssim3f_chunks_inputs.py):
  17 x 17 x 131   four tiles, three of them one voxel wide or high; 16 full cells and a 3-slice cell; at depth 64 the last chunk is 3
                  slices long.  Must cover depths 8, 16, 32, 64 and the single chunk of the whole depth (17 cells in one workgroup).
  5 x 3 x 1000    both lateral axes shorter than the window, under deep chunks (up to 64 cells per workgroup).  Must cover at least
                  two depths of 128 or more.
Each test computes, with tests/ssim3f_plan.py (which tests/test_ssim3f_plan_cpu.py holds to the C++ planner) at the device's CU count,
the smallest count of at most 512 volumes that gives each depth, prints the depth and the cells per workgroup of every launch and fails,
never skips, when the depths above are not covered.  On 256 CUs: 1, 16, 31, 61 and 154 volumes; 1, 9, 17, 33, 97, 193 and 449 volumes.

Inputs.  Seven distinct seeded pairs per shape, uploaded once; a launch's descriptors pick among them, and every volume's dLoss/dS among
five values, by a seeded draw in which neighbours differ: a volume-index mix-up in the descriptors, the gOut vector, the partials or the
coefficient scratch shows (identical volumes would hide all four).  The first, a middle and the last volume of a launch get a map, each
in a layout of its own (dense, step 2, negative sliceStride), pre-filled with a sentinel; the other volumes get none.  Every gradient
volume lies in one buffer with sentinel gaps.  Before each checked launch a launch of the same count over another draw leaves other
data in the partials and the coefficient scratch; its sums are checked as well.  The deepest launch of each shape runs once more with dA
alone and once with dB alone.

The launch limit: 65537 volumes of 2 x 1 x 3 in one call, forward and gradient -- two sub-batches, 65535 and 2 volumes -- drawn from 7
pairs x 5 gOut values: every sum and every gradient volume has the bits of its combination launched alone (35 lone launches).

The ring: 2 * kSfSlots + 1 = 17 different pairs of 33 x 17 x 9, one forward and one gradient enqueue each (a gradient enqueue puts two
tables in one slot), back to back, one synchronise: the blocking device call and the lone gradient of each pair, bit for bit.

After a return code that is neither success nor EINVAL the module starts nothing more on the GPU (test_gpu_ssimk's _device_error, shared
with that module).  Every test frees its own buffers.  The module prints its wall time and its peak device memory when it ends.

Cost, measured on an MI355X: the 6 tests take 1.5 s together, no test more than 0.3 s; the device holds 174 MiB more than before the
module at the peak (the deepest launch: 449 volumes of 5 x 3 x 1000 are 6.7 M voxels, 108 MB of coefficient scratch, which the module
trims when it ends, and 54 MB of gradient volumes).  The module prints both figures when it ends.
"""
import ctypes
import re
import time

import numpy as np
import pytest

import ssim3f_chunks_inputs as IN
import ssim3f_model as S
import ssim3f_plan as P
import ssim_amd
from ssim3f_chunks_inputs import RANGE
from test_gpu_ssim3f import SENT, Vol
from test_gpu_ssimk import _device_error

pytestmark = pytest.mark.gpu

PX_TOL, G_TOL, GRAD_TOL, _ = S.tolerances()
GAP = 64                                                   # sentinel floats between the gradient volumes of a launch
FILL64 = np.float64(-777.0)
MAP_LAYOUTS = ("dense", "step 2", "negative sliceStride")  # of the first, a middle and the last volume of a launch
BY_SHAPE = pytest.mark.parametrize("shape", IN.SHAPES, ids=IN.shape_id)


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


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- the device, the clock and the memory --------------------------------------------------------------------------------------------

class Device(object):
    def __init__(self, ctx):
        self.ctx, self.t0 = ctx, time.time()
        said = re.search(r"(\d+) CUs", ctx.describe())
        assert said, ctx.describe()
        self.cus = int(said.group(1))
        assert self.cus > 0 and ssim_amd.get_plan(64, 64, 1, ctx).waveSlots % (4 * self.cus) == 0, (self.cus, ctx.describe())
        self.free0 = self.min_free = ssim_amd.memory_info(ctx)[0]
        self.refs = {}

    def sample(self):
        self.min_free = min(self.min_free, ssim_amd.memory_info(self.ctx)[0])

    def close(self):
        self.ctx.trim()
        print("\nvolume chunks: %d CUs; module wall time %.1f s; peak device memory in use by the module %.1f MiB" % (
            self.cus, time.time() - self.t0, (self.free0 - self.min_free) / 2.0 ** 20))


@pytest.fixture(scope="module")
def device(gpu_ctx):
    d = Device(gpu_ctx)
    yield d
    d.close()


# ---- one launch ----------------------------------------------------------------------------------------------------------------------

class Inputs(object):
    """The pairs of one shape in device memory, dense."""

    def __init__(self, ctx, shape, pairs):
        assert not _device_error, "an earlier call left a device error: %r" % _device_error
        self.shape, self.bufs = shape, []
        for a, b in pairs:
            self.bufs.append((ctx.upload(a), ctx.upload(b)))

    def params(self, k, map_ptr=None, map_strides=None):
        w, h, d = self.shape
        a, b = self.bufs[k]
        return ssim_amd.make_params3f(w, h, d, a.ptr, (1, w, w * h), b.ptr, (1, w, w * h), map_ptr, map_strides)

    def free(self):
        for a, b in self.bufs:
            a.free()
            b.free()


def launch(device, inp, pick, g_values, which=3, map_at=(), read_grads=True):
    """ONE forward enqueue and ONE gradient enqueue of len(pick) volumes -- volume i is pair pick[i] with dLoss/dS = g_values[i] --, one
    synchronise.  map_at: {volume: layout} of the volumes that get a map.  Returns (sums as float64 [n], {volume: map}, gradients as
    float32 [n, sides, D, H, W] -- sides: dA and dB, or the one of `which` -- or None).  Every sentinel around the sums and between the
    gradient volumes is asserted untouched, every map voxel written and every float outside the maps untouched (Vol.result)."""
    ctx, (w, h, d), n = device.ctx, inp.shape, len(pick)
    vox, sides = w * h * d, (2 if which == 3 else 1)
    per = vox + GAP
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    bufs, maps = [], dict((i, Vol(ctx, (d, h, w), lay)) for i, lay in dict(map_at).items())
    try:
        fresh = np.full(sides * n * per + GAP, SENT, np.float32)
        out = ctx.upload(fresh)
        sums = ctx.upload(np.full(n + 2, FILL64))
        go = ctx.upload(np.asarray(g_values, np.float32).reshape(n))
        bufs += [out, sums, go]
        ps = (ssim_amd.Params3F * n)()
        grads = [(ssim_amd.Grad3F * n)() if which & (1 << k) else None for k in range(2)]
        for i, k in enumerate(pick):
            m = maps.get(i)
            ps[i] = inp.params(int(k), m.ptr if m else None, m.strides if m else None)
            for side, arr in enumerate(g for g in grads if g is not None):
                arr[i] = ssim_amd.Grad3F(out.ptr + 4 * (GAP + (sides * i + side) * per), 1, w, w * h)
        call(ctx.enqueue_ssim3f, ps, n, RANGE, sums.ptr + 8)
        call(ctx.enqueue_ssim3f_grad, ps, n, RANGE, go.ptr, grads[0], grads[1])
        call(ctx.synchronize)
        device.sample()
        s = sums.download(np.float64, (n + 2,))
        assert s[0] == FILL64 and s[-1] == FILL64, "a double beside the sums was written"
        got_maps = dict((i, m.result()) for i, m in maps.items())
        g = None
        if read_grads:
            host = out.download(np.float32, fresh.shape)
            body = host[GAP:].reshape(sides * n, per)
            assert np.all(host[:GAP] == SENT) and np.all(body[:, vox:] == SENT), "a gap between the gradient volumes changed"
            g = body[:, :vox].reshape(n, sides, d, h, w)
        return s[1:-1].copy(), got_maps, g
    finally:
        for x in bufs + list(maps.values()):
            x.free()


# ---- the one-volume references -------------------------------------------------------------------------------------------------------

def references(device, shape, inp):
    """Every pair launched ALONE (chunks of 8 slices, asserted): its fp64 sum, its dense map, and both gradients for each of the five
    gOut values -- sums [7], maps [7], gradients [7, 5, 2, D, H, W]; computed once per shape."""
    if shape in device.refs:
        return device.refs[shape]
    w, h, d = shape
    one = P.plan3f(w, h, d, 1, device.cus)
    assert one.chunk_slices == P.CELL_Z, "one volume alone does not run at depth 8: %s" % P.describe(one, w, h, d, 1)
    sums, maps, grads = np.zeros(IN.PAIRS), [], np.zeros((IN.PAIRS, len(IN.G_OUTS), 2, d, h, w), np.float32)
    for k in range(IN.PAIRS):
        for g, g_out in enumerate(IN.G_OUTS):
            s, m, gr = launch(device, inp, [k], [g_out], map_at={0: "dense"} if g == 0 else ())
            if g == 0:
                sums[k] = s[0]
                maps.append(m[0])
            else:
                assert s.view(np.uint64)[0] == sums[k:k + 1].view(np.uint64)[0], (shape, k, g)
            grads[k, g] = gr[0]
    device.refs[shape] = (sums, maps, grads)
    return device.refs[shape]


@BY_SHAPE
def test_one_volume_alone_meets_the_model(device, shape):
    """All seven pairs: value and map, and both gradients at one gOut value each, at ssim3f_model.tolerances()."""
    inp = Inputs(device.ctx, shape, IN.pairs(shape))
    try:
        sums, maps, grads = references(device, shape, inp)
    finally:
        inp.free()
    vox = S.voxels(shape[::-1])
    for k in range(IN.PAIRS):
        g = IN.held_g(k)
        (gv, gm), want = IN.model(shape, k), IN.model_grad(shape, k, g)
        e_px, e_g = float(np.abs(maps[k].astype(np.float64) - gm).max()), abs(sums[k] / vox - gv)
        e_grad = [float(np.abs(grads[k, g, side] - want[side]).max() / np.abs(want[side]).max()) for side in range(2)]
        print("%s pair %d alone: per voxel %.3g (bound %.3g), global %.3g (bound %.3g), gradients at gOut %g: %.3g %.3g of max|grad| (bound %.3g)" % (
            IN.shape_id(shape), k, e_px, PX_TOL, e_g, G_TOL, IN.G_OUTS[g], e_grad[0], e_grad[1], GRAD_TOL))
        assert np.all(np.isfinite(maps[k])) and np.all(np.isfinite(grads[k])), (shape, k)
        assert e_px <= PX_TOL and e_g <= G_TOL and max(e_grad) <= GRAD_TOL, (shape, k, e_px, e_g, e_grad)
    # the five gOut values give five different gradients
    assert len(set(grads[0, g].tobytes() for g in range(len(IN.G_OUTS)))) == len(IN.G_OUTS)


# ---- every chunk depth ---------------------------------------------------------------------------------------------------------------

def differing(got, want):
    """Volumes whose bits differ."""
    return np.flatnonzero(np.any((u32(got) != u32(want)).reshape(len(got), -1), axis=1))


def check_launch(device, inp, refs, n, salt, what, which=3, with_maps=True, read_grads=True):
    """One launch of n volumes over the draw `salt` against the one-volume launches: every sum; the maps of the first, a middle and the
    last volume; every gradient volume."""
    sums, maps, grads = refs
    pick, gpick = IN.picks(n, salt)
    at = sorted(set((0, n // 2, n - 1))) if with_maps else []
    got_s, got_m, got_g = launch(device, inp, pick, [IN.G_OUTS[g] for g in gpick], which, dict(zip(at, MAP_LAYOUTS)), read_grads)
    bad = np.flatnonzero(got_s.view(np.uint64) != sums[pick].view(np.uint64))
    assert len(bad) == 0, "%s: %d of %d fp64 sums differ from the volume launched alone; the first: volume %d (pair %d): %r, alone %r" % (
        what, len(bad), n, bad[0], pick[bad[0]], got_s[bad[0]], sums[pick[bad[0]]])
    for i, m in sorted(got_m.items()):
        diff = np.argwhere(u32(m) != u32(maps[pick[i]]))
        assert len(diff) == 0, "%s: the map of volume %d (pair %d) differs from the one of the volume launched alone in %d of %d voxels, the first at (z, y, x) = %s" % (
            what, i, pick[i], len(diff), m.size, tuple(diff[0]))
    if read_grads:
        want = grads[pick, gpick] if which == 3 else grads[pick, gpick, which - 1:which]
        bad = differing(got_g, want)
        assert len(bad) == 0, "%s: the gradients of %d of %d volumes differ from the ones of the volume launched alone; the first: volume %d (pair %d, gOut %g)" % (
            what, len(bad), n, bad[0], pick[bad[0]], IN.G_OUTS[gpick[bad[0]]])
    return pick


@BY_SHAPE
def test_every_chunk_depth_has_the_bits_of_the_volume_alone(device, shape):
    w, h, d = shape
    launches = IN.depth_counts(shape, device.cus)
    print()
    for n, geo in launches:
        print("on %d CUs: %s" % (device.cus, P.describe(geo, w, h, d, n)))
    depths = [geo.chunk_slices for _, geo in launches]
    if shape == IN.SHAPES[0]:
        assert set(depths) >= {8, 16, 32, 64} and any(geo.chunks == 1 for _, geo in launches), "17 x 17 x 131 does not cover depths 8, 16, 32, 64 and the whole depth: %r" % depths
        assert any(P.cells_per_workgroup(geo, d) > 4 for _, geo in launches)
    else:
        assert len([x for x in depths if x >= 128]) >= 2, "5 x 3 x 1000 does not cover two depths of 128 or more: %r" % depths
    inp = Inputs(device.ctx, shape, IN.pairs(shape))
    try:
        refs = references(device, shape, inp)
        for j, (n, geo) in enumerate(launches):
            what = "%s, %d volumes, chunks of %d slices" % (IN.shape_id(shape), n, geo.chunk_slices)
            # another draw first: the partials and the coefficient scratch then hold other volumes' data
            other = check_launch(device, inp, refs, n, 2 * j + 1, what + ", the launch before", with_maps=False, read_grads=False)
            pick = check_launch(device, inp, refs, n, 2 * j, what)
            assert np.any(pick != other)
        n, geo = launches[-1]
        for which in (1, 2):
            check_launch(device, inp, refs, n, 100 + which, "%s, %d volumes, chunks of %d slices, %s alone" % (IN.shape_id(shape), n, geo.chunk_slices, ("dA", "dB")[which - 1]),
                         which=which, with_maps=False)
    finally:
        inp.free()


# ---- the launch limit ----------------------------------------------------------------------------------------------------------------

def test_a_call_beyond_the_launch_limit_is_cut_without_a_trace(device):
    """65537 volumes of 2 x 1 x 3 in one forward and one gradient call: sub-batches of 65535 and 2 volumes."""
    ctx, shape, n = device.ctx, IN.LIMIT_SHAPE, IN.LIMIT_COUNT
    w, h, d = shape
    vox, combos = w * h * d, IN.PAIRS * len(IN.G_OUTS)
    for scratch in (P.forward_scratch(w, h, d), P.grad_scratch(w, h, d, 3)):
        assert P.sub_batches(w, h, d, n, scratch) == [(0, 65535), (65535, 2)]
    assert P.plan3f(w, h, d, 1, device.cus).chunk_slices == P.CELL_Z
    pick, gpick = IN.picks(n, IN.LIMIT_SALT)
    assert len(set(zip(pick.tolist(), gpick.tolist()))) == combos and gpick[65535] != gpick[0] and gpick[65536] != gpick[1]
    inp = Inputs(ctx, shape, IN.pairs(shape))
    bufs = []
    try:
        # the 35 combinations, each launched alone
        sums, grads = np.zeros(IN.PAIRS), np.zeros((IN.PAIRS, len(IN.G_OUTS), 2, d, h, w), np.float32)
        for k in range(IN.PAIRS):
            for g, g_out in enumerate(IN.G_OUTS):
                s, _, gr = launch(device, inp, [k], [g_out])
                assert g == 0 or s.view(np.uint64)[0] == sums[k:k + 1].view(np.uint64)[0]
                sums[k], grads[k, g] = s[0], gr[0]
            gv, _ = S.ssim(*IN.pairs(shape)[k], RANGE)
            assert abs(sums[k] / vox - gv) <= G_TOL, (k, sums[k] / vox, gv)
        assert len(set(grads[k, g].tobytes() for k in range(IN.PAIRS) for g in range(len(IN.G_OUTS)))) == combos
        # the call: descriptors and gradient volumes filled through numpy views of the ctypes arrays; every gradient has 6 floats of
        # its own in one buffer, 2 sentinel floats before each
        assert not _device_error, "an earlier call left a device error: %r" % _device_error
        per = vox + 2
        fresh = np.full(2 * n * per + 2, SENT, np.float32)
        out, sm = ctx.upload(fresh), ctx.upload(np.full(n + 2, FILL64))
        go = ctx.upload(np.float32(IN.G_OUTS)[gpick])
        bufs += [out, sm, go]
        ps, ga, gb = (ssim_amd.Params3F * n)(), (ssim_amd.Grad3F * n)(), (ssim_amd.Grad3F * n)()
        assert ctypes.sizeof(ps) == n * np.dtype(ssim_amd.Params3F).itemsize and ctypes.sizeof(ga) == n * np.dtype(ssim_amd.Grad3F).itemsize
        pv = np.frombuffer(ps, np.dtype(ssim_amd.Params3F))
        one = np.frombuffer((ssim_amd.Params3F * IN.PAIRS)(*[inp.params(k) for k in range(IN.PAIRS)]), np.dtype(ssim_amd.Params3F))
        pv[:] = one[pick]
        for side, arr in enumerate((ga, gb)):
            gv = np.frombuffer(arr, np.dtype(ssim_amd.Grad3F))
            gv["topLeft"] = out.ptr + 4 * (2 + (2 * np.arange(n, dtype=np.uint64) + side) * per)
            gv["step"], gv["stride"], gv["sliceStride"] = 1, w, w * h
        assert (ps[n - 1].imgA.topLeft, ps[n - 1].depth) == (inp.bufs[pick[n - 1]][0].ptr, d) and gb[n - 1].topLeft == out.ptr + 4 * (2 + (2 * n - 1) * per)
        assert gb[n - 1].topLeft + 4 * vox + 8 == out.ptr + fresh.nbytes and (gb[n - 1].step, gb[n - 1].stride, gb[n - 1].sliceStride) == (1, w, w * h)
        call(ctx.enqueue_ssim3f, ps, n, RANGE, sm.ptr + 8)
        call(ctx.enqueue_ssim3f_grad, ps, n, RANGE, go.ptr, ga, gb)
        call(ctx.synchronize)
        device.sample()
        s = sm.download(np.float64, (n + 2,))
        assert s[0] == FILL64 and s[-1] == FILL64, "a double beside the sums was written"
        bad = np.flatnonzero(s[1:-1].view(np.uint64) != sums[pick].view(np.uint64))
        assert len(bad) == 0, "%d of %d fp64 sums differ from the volume launched alone; the first: volume %d (pair %d): %r, alone %r" % (
            len(bad), n, bad[0], pick[bad[0]], s[1 + bad[0]], sums[pick[bad[0]]])
        host = out.download(np.float32, fresh.shape)
        body = host[2:].reshape(2 * n, per)
        assert np.all(host[:2] == SENT) and np.all(body[:, vox:] == SENT), "a gap between the gradient volumes changed"
        bad = differing(body[:, :vox].reshape(n, 2, vox), grads[pick, gpick].reshape(n, 2, vox))
        assert len(bad) == 0, "the gradients of %d of %d volumes differ from the ones of the volume launched alone; the first: volume %d (pair %d, gOut %g)" % (
            len(bad), n, bad[0], pick[bad[0]], IN.G_OUTS[gpick[bad[0]]])
    finally:
        for x in bufs:
            x.free()
        inp.free()


# ---- the ring ------------------------------------------------------------------------------------------------------------------------

def test_volume_enqueues_beyond_the_ring_keep_their_order(device):
    """17 different pairs of 33 x 17 x 9: one forward and one gradient enqueue each, back to back -- 34 launches from a ring of 8 slots,
    every second one with two tables in its slot -- and one synchronise."""
    ctx, shape, n = device.ctx, IN.RING_SHAPE, IN.RING_COUNT
    w, h, d = shape
    vox = w * h * d
    pairs = IN.pairs(shape, n)
    assert len(set(a.tobytes() for a, _ in pairs)) == n
    g_out = np.float32([IN.G_OUTS[i % len(IN.G_OUTS)] for i in range(n)])
    inp = Inputs(ctx, shape, pairs)
    bufs = []
    try:
        blocks = []
        for i in range(n):
            ps = (ssim_amd.Params3F * 1)()
            ps[0] = inp.params(i)
            blocks.append(ps)
        want_v = [call(ctx.ssim3f_device, ps, 1, RANGE) for ps in blocks]
        assert len(set(v.tobytes() for v in want_v)) > 1
        want_g = np.array([launch(device, inp, [i], [g_out[i]])[2][0] for i in range(n)])
        assert not _device_error, "an earlier call left a device error: %r" % _device_error
        per = vox + GAP
        fresh = np.full(2 * n * per + GAP, SENT, np.float32)
        out, sums, go = ctx.upload(fresh), ctx.upload(np.full(n + 2, FILL64)), ctx.upload(g_out)
        bufs += [out, sums, go]
        keep = []
        for i, ps in enumerate(blocks):
            ga, gb = (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)()
            ga[0] = ssim_amd.Grad3F(out.ptr + 4 * (GAP + 2 * i * per), 1, w, w * h)
            gb[0] = ssim_amd.Grad3F(out.ptr + 4 * (GAP + (2 * i + 1) * per), 1, w, w * h)
            keep.append((ga, gb))
            call(ctx.enqueue_ssim3f, ps, 1, RANGE, sums.ptr + 8 * (1 + i))
            call(ctx.enqueue_ssim3f_grad, ps, 1, RANGE, go.ptr + 4 * i, ga, gb)
        call(ctx.synchronize)
        device.sample()
        s = sums.download(np.float64, (n + 2,))
        assert s[0] == FILL64 and s[-1] == FILL64
        for i in range(n):
            assert np.float32(s[1 + i] / np.float64(S.voxels((d, h, w)))).tobytes() == want_v[i].tobytes(), (i, s[1 + i], float(want_v[i][0]))
        host = out.download(np.float32, fresh.shape)
        body = host[GAP:].reshape(2 * n, per)
        assert np.all(host[:GAP] == SENT) and np.all(body[:, vox:] == SENT), "a gap between the gradient volumes changed"
        bad = differing(body[:, :vox].reshape(n, 2, vox), want_g.reshape(n, 2, vox))
        assert len(bad) == 0, "the gradients of pairs %s differ from the lone gradient" % bad.tolist()
    finally:
        for x in bufs:
            x.free()
        inp.free()
