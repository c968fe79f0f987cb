"""GPU: strips of many reduction cells in the strip kernels of the five sample families (ssim16, ssimf, ssimh, msssimf and the windowed
ssimk kernels), and the windowed gradient kernels in launches of hundreds of pairs: every pair of a large launch must have, bit for bit,
the sum and the map it has when it is launched alone.

Why.  A strip walks its rows one reduction cell at a time, parks one fp64 leaf per cell and flushes the cells eight at a time; the flush
advances cell_y, colsum is zeroed per cell, the image's last cell may be short or odd (ROW_LAST).  The planners give a launch that fits
one round of wave slots strips of ONE cell, and every small shape of the other modules fits one round: their strips never hold a second
cell.  Strip height is scheduling only -- cells sit at absolute positions -- so a launch of many pairs, which makes the planner choose tall
strips, must reproduce the one-pair launch (single-cell strips, asserted), and the one-pair launch is held to the float64 models at the
bounds the families' own modules assert.  No bound is new.

Cases (W x H, pairs; the geometry on 256 CUs -- each case computes it for the device's CU count with tests/sample_plan.py, which
tests/test_sample_plan_cpu.py holds to the C++ planners, prints it and fails, never skips, when its conditions do not hold):
  A    9 x 603, 1000   strips of 208 rows = 26 cells of 8: three full batch flushes, then 2 cells; three strips per column, the last
                       187 rows = 23 cells and a 3-row cell.  Needs >= 9 cells per strip, >= 2 strips per column, a short last cell.
                       Run with three maps and once more with no map at all (the MAP = 0 kernels).
  B    9 x 2115, 1000  32-row cells, strips of 736 rows = 23 cells, the last 643 rows = 20 cells and a 3-row cell.  Same conditions.
  C    260 x 601, 350  strips of 56 rows = 7 cells, never a full batch; three strip columns, the third 4 pixels wide; 11 strips per
                       column, the last 41 rows = 5 cells and a 1-row cell: ROW_LAST with no row pair before it.  Needs 2 .. 7 cells per
                       strip, >= 3 strip columns, a last cell of 1 row.  The width is even and the maps dense: the MAP = 2 kernels.
  msssimf is held to the conditions at scale 0; the coarser scales are printed.

Inputs (tests/tall_strips_inputs.py).  Seven distinct seeded pairs per shape and sample type, uploaded once; the launch's descriptors
pick among them by a seeded draw, so an image-index mix-up or a stale partial shows (identical pairs would hide both).  Three pairs of a
launch -- the first, the middle one and the last -- get a map plane of their own, pre-filled with a sentinel, the others none: the empty
buffer resource of the 32-bit map form, a thousand times.  Before the launch that is checked for maps, a launch of the same count over
another draw leaves other data in the scratch partials (its sums are checked as well).

The windowed gradient kernels have otherwise never seen more than 3 pairs: per window one launch of 300 pairs at 9 x 603 for the scalar
upstream form and one for the per-pixel form, 600 gradient planes each, every plane bit for bit the one-pair gradient, which meets the model.

After any device error the module starts nothing more on the GPU (test_gpu_ssimk's _ok / _device_error, shared with that module).

Cost, measured on an MI355X: the 61 tests take 2.4 s together; the device holds 218 MiB more than before the module at the peak (most of it the context's
grow-only scratch: the pyramids of 350 msssimf pairs of 260 x 601 are 146 MB; the module trims it when it ends); every test frees its own
buffers.  The module prints both figures when it ends.
"""
import ctypes
import re
import time

import numpy as np
import pytest

import halfmodel as HM
import msssimf_model as MS
import sample_plan as SP
import ssimf_model as MF
import ssimk_model as K
import ssim_amd
import tall_strips_inputs as T
from tall_strips_inputs import RANGE
from test_gpu_sample_forms import FAMS, SSIMF, assert_same_bits, launch
from test_gpu_ssim16 import G_TOL as G16_TOL, PX_TOL as PX16_TOL
from test_gpu_ssimk import _device_error, _ok, _sync, _wref, backward, forward, mk
from test_gpu_ssimw import FILL32, Plane

pytestmark = pytest.mark.gpu

# (step, flip) of the three map planes of a case: first pair, middle pair, last pair.  A and B have an odd width (form MAP = 1 whatever
# the step: interleaved and reversed planes, whose gaps Plane.read checks); C stays dense, which an even width turns into form MAP = 2.
MAP_LAYOUTS = {"A": ((1, False), (3, False), (2, True)), "B": ((1, False), (2, True), (1, True)), "C": ((1, False), (1, False), (1, False))}
GAP = 64                                                   # sentinel floats between the gradient planes of a launch


class Win(object):
    """One window of ssimk_model.WINDOWS, driven as test_gpu_sample_forms.Fam drives a family (kind "k")."""
    kind, maps = "k", True

    def __init__(self, window):
        self.window, self.name = window, "ssimk/" + K.name_of(window).replace(" ", "-")

    def make(self, w, h, ia, ib, m=None):
        if m is None:
            return ssim_amd.make_params_f(w, h, *(ia + ib))
        return ssim_amd.make_params_f(w, h, *(ia + ib), map_ptr=m[0], map_step=m[1], map_stride=m[2])

    def __repr__(self):
        return self.name


RUNNERS = list(FAMS) + [Win(window) for window in K.WINDOWS]
BY_RUNNER = pytest.mark.parametrize("run", RUNNERS, ids=repr)
BY_CASE = pytest.mark.parametrize("case", T.CASES, ids=[c[0] for c in T.CASES])


def host_pairs(run, shape):
    """The seven pairs in the family's sample type."""
    if run.kind == "16":
        return T.pairs_16(shape, run.depth)
    if run.kind == "h":
        return [u for u, _ in T.pairs_h(shape, run.enc)]
    return T.pairs_f(shape)


def plan_of(run, w, h, n, cus):
    if run.kind == "k":
        return SP.plank(K.radius(run.window), w, h, n, cus)
    return {"f": SP.planf, "16": SP.plan16, "h": SP.planh, "ms": SP.planms}[run.kind](w, h, n, cus)


def run_launch(ctx, run, plist):
    """One enqueue of the pairs `plist`: a row per pair -- the fp64 sum; msssimf: the fp64 value and the scales x 2 means."""
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    if run.kind != "k":
        try:
            return launch(ctx, run, plist)
        except ssim_amd.SsimError as e:
            if e.errno != 22:
                _device_error.append(e.errno)
            raise
    n = len(plist)
    ps = (ssim_amd.ParamsF * n)(*plist)
    sums = ctx.upload(np.full(n, np.nan))
    try:
        _ok(ctx.lib.rmgr_ssim_hip_enqueue_ssimf_win(ctx.handle, n, ps, RANGE, _wref(mk(run.window)), sums.ptr))
        _sync(ctx)
        return sums.download(np.float64, (n, 1))
    finally:
        sums.free()


# ---- the device, the clock and the memory --------------------------------------------------------------------------------------------

class Device(object):
    def __init__(self, ctx):
        self.ctx, self.t0 = ctx, time.time()
        mode = ctypes.c_int32(-1)
        assert ctx.lib.rmgr_ssim_hip_get_mode(ctx.handle, ctypes.byref(mode)) == 0
        # waveSlots of rmgr_ssim_hip_get_plan: CUs x 4 SIMDs x the waves per SIMD of the context's mode (tests/test_abi_cpu.py: 2048 = 256 x 4 x 2)
        waves = 3 if mode.value in (ssim_amd.MODE_DOUBLE, ssim_amd.MODE_SEPARABLE) else 2
        slots = ssim_amd.get_plan(64, 64, 1, ctx).waveSlots
        self.cus = slots // (4 * waves)
        said = re.search(r"(\d+) CUs", ctx.describe())
        assert self.cus > 0 and slots == self.cus * 4 * waves and said and int(said.group(1)) == self.cus, (slots, mode.value, ctx.describe())
        self.free0 = self.min_free = ssim_amd.memory_info(ctx)[0]
        self.refs = {}

    def sample(self):
        self.min_free = min(self.min_free, ssim_amd.memory_info(self.ctx)[0])

    def close(self):
        self.ctx.trim()
        print("\ntall strips: %d CUs; module wall time %.1f s; peak device memory in use by the module %.1f MiB" % (
            self.cus, time.time() - self.t0, (self.free0 - self.min_free) / 2.0 ** 20))


@pytest.fixture(scope="module")
def device(gpu_ctx):
    d = Device(gpu_ctx)
    yield d
    d.close()


# ---- the one-pair references ---------------------------------------------------------------------------------------------------------

def hold_to_the_model(ctx, run, shape, k, row, m):
    """One one-pair result (its row of run_launch and its map, None for msssimf) against the family's float64 model at the bounds of its
    own GPU module; the half family against ssimf on the widened planes, bit for bit.  Returns (per pixel or per mean, global, bounds)."""
    h, w = shape
    if run.kind == "h":
        fa, fb = T.pairs_h(shape, run.enc)[k][1]
        da, db, wm = ctx.upload(fa), ctx.upload(fb), Plane(ctx, np.full(shape, FILL32, np.float32), fill=FILL32)
        try:
            wide = run_launch(ctx, SSIMF, [SSIMF.make(w, h, (da.ptr, 1, w), (db.ptr, 1, w), (wm.ptr, wm.dstep, wm.dstride))])[0]
            wide_map = wm.read()
        finally:
            for x in (da, db, wm):
                x.free()
        assert row.view(np.uint64)[0] == wide.view(np.uint64)[0], (run, shape, k, "sum differs from ssimf on the widened planes", row, wide)
        assert HM.same_f32(m, wide_map), (run, shape, k, "map differs from ssimf on the widened planes")
        return 0, 0, (0, 0)
    if run.kind == "ms":
        gv, gm = T.model_ms(shape, k, run.scales, run.weights)
        px, g, bound = float(np.abs(row[1:].reshape(run.scales, 2) - gm).max()), abs(float(row[0]) - gv), (MS.MEAN_TOL, MS.VALUE_TOL)
    elif run.kind == "k":
        gv, gm = T.model_k(shape, k, run.window)
        px, g, bound = float(np.abs(m - gm).max()), abs(float(row[0]) / (float(w) * float(h)) - gv), K.tolerances(run.window)[:2]
    else:
        gv, gm = T.model_f(shape, k) if run.kind == "f" else T.model_16(shape, run.depth, k)
        bound = (MF.PX_TOL, MF.G_TOL) if run.kind == "f" else (PX16_TOL, G16_TOL)
        px, g = float(np.abs(m.astype(np.float64) - gm).max()), abs(float(np.float32(row[0] / (float(w) * float(h)))) - gv)
    assert (m is None or np.all(np.isfinite(m))) and px <= bound[0] and g <= bound[1], (run, shape, k, px, g, bound)
    return px, g, bound


def references(device, run, shape, dev):
    """(rows, maps) of the seven pairs, each launched ALONE (single-cell strips, asserted by the caller) and held to its model: computed
    once per family and shape.  dev: the pairs' device planes.  The windows go through test_gpu_ssimk.forward, planes of its own."""
    key = (run.name, shape)
    if key in device.refs:
        return device.refs[key]
    ctx, (h, w) = device.ctx, shape
    rows, maps, worst = [], [], (0, 0, None)
    for k in range(T.PAIRS):
        if run.kind == "k":
            assert not _device_error, "an earlier call left a device error: %r" % _device_error
            sums, ms = forward(ctx, [T.pairs_f(shape)[k]], RANGE, mk(run.window))
            row, m = np.array([sums[0]], np.float64), ms[0]
        elif run.maps:
            p = Plane(ctx, np.full(shape, FILL32, np.float32), fill=FILL32)
            try:
                row = run_launch(ctx, run, [run.make(w, h, dev[k][0], dev[k][1], (p.ptr, p.dstep, p.dstride))])[0]
                m = p.read()
            finally:
                p.free()
        else:
            row, m = run_launch(ctx, run, [run.make(w, h, dev[k][0], dev[k][1])])[0], None
        px, g, bound = hold_to_the_model(ctx, run, shape, k, row, m)
        worst = (max(worst[0], px), max(worst[1], g), bound)
        rows.append(row)
        maps.append(m)
    print("%s %s alone: worst per pixel (msssimf: per mean) %.3g (bound %.3g), global %.3g (bound %.3g)" % (
        run, T.shape_id(shape), worst[0], worst[2][0], worst[1], worst[2][1]))
    device.refs[key] = (np.array(rows), maps if run.maps else None)
    return device.refs[key]


# ---- the launches of many pairs ------------------------------------------------------------------------------------------------------

def check_conditions(run, case, cus):
    name, w, h, n = case
    geo = plan_of(run, w, h, n, cus)
    what = "%s, case %s on %d CUs: %s" % (run, name, cus, SP.describe(geo, w, h, n))
    print(what)
    if run.kind == "ms":
        for s in range(1, run.scales):
            sw, sh = SP.msf_dim(w, s), SP.msf_dim(h, s)
            print("    scale %d: %s" % (s, SP.describe(SP.planms(w, h, n, cus, s), sw, sh, n)))
    cells = SP.cells_per_strip(geo, h)
    if name in ("A", "B"):
        assert cells > SP.CELL_BATCH and geo.strips_y >= 2 and SP.last_cell_rows(geo, h) < geo.cell_rows, what
        assert geo.cell_rows == (32 if name == "B" else 8), what
    else:
        assert 2 <= cells < SP.CELL_BATCH and geo.strips_x >= 3 and SP.last_cell_rows(geo, h) == 1, what
    one = plan_of(run, w, h, 1, cus)
    assert SP.cells_per_strip(one, h) == 1, "%s: one pair alone is not single-cell strips: %s" % (run, SP.describe(one, w, h, 1))


def same_rows(run, got, rows, pick, what):
    want = rows[pick]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, "%s, %s: %d of %d fp64 results (%d of %d pairs) differ from the pair launched alone; the first: pair %d (image %d), column %d: %r, alone %r" % (
        run, what, len(bad), got.size, len(set(bad[:, 0].tolist())), len(got), bad[0][0], pick[bad[0][0]], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


def tall_launch(device, run, case, with_maps):
    ctx, (name, w, h, n), shape = device.ctx, case, (case[2], case[1])
    check_conditions(run, case, device.cus)
    bufs, planes = [], {}
    try:
        dev = []
        for a, b in host_pairs(run, shape):
            da, db = ctx.upload(a), ctx.upload(b)
            bufs += [da, db]
            dev.append(((da.ptr, 1, w), (db.ptr, 1, w)))
        rows, maps = references(device, run, shape, dev)
        salt = 10 * "ABC".index(name) + (0 if with_maps else 5)
        # another draw first: the scratch partials then hold other pairs' cells
        other = T.picks(n, salt + 1)
        got = run_launch(ctx, run, [run.make(w, h, *dev[k]) for k in other])
        same_rows(run, got, rows, other, "case %s, the launch before, no map" % name)
        pick = T.picks(n, salt)
        assert np.any(pick != other)
        if with_maps and run.maps:
            for i, (step, flip) in zip((0, n // 2, n - 1), MAP_LAYOUTS[name]):
                planes[i] = Plane(ctx, np.full(shape, FILL32, np.float32), step=step, flip=flip, fill=FILL32)
        plist = []
        for i, k in enumerate(pick):
            p = planes.get(i)
            plist.append(run.make(w, h, dev[k][0], dev[k][1], (p.ptr, p.dstep, p.dstride) if p is not None else None))
        got = run_launch(ctx, run, plist)
        device.sample()
        same_rows(run, got, rows, pick, "case %s, %s" % (name, "three maps" if planes else "no map"))
        for i, p in sorted(planes.items()):
            m = p.read()                                  # asserts that the gaps of an interleaved plane still hold the sentinel
            assert_same_bits(m, maps[pick[i]], "%s, case %s: the map of pair %d (image %d)" % (run, name, i, pick[i]))
    finally:
        for x in bufs + list(planes.values()):
            x.free()


@BY_CASE
@BY_RUNNER
def test_every_pair_of_a_tall_strip_launch_has_the_bits_it_has_alone(device, run, case):
    tall_launch(device, run, case, with_maps=True)


@pytest.mark.parametrize("run", [r for r in RUNNERS if r.maps], ids=repr)
def test_case_a_without_any_map(device, run):
    tall_launch(device, run, T.CASES[0], with_maps=False)


# ---- the windowed gradient kernels in a launch of 300 pairs --------------------------------------------------------------------------

@pytest.mark.parametrize("window", K.WINDOWS, ids=K.name_of)
def test_window_gradients_of_300_pairs_have_the_bits_of_the_one_pair_gradients(device, window):
    ctx, shape, n = device.ctx, T.GRAD_SHAPE, T.GRAD_COUNT
    h, w = shape
    win, grad_tol = mk(window), K.tolerances(window)[2]
    pairs, ups = T.pairs_f(shape), T.upstream(shape)
    # the one-pair gradients, held to the model
    alone, worst = [], 0.0
    for k in range(T.PAIRS):
        assert not _device_error, "an earlier call left a device error: %r" % _device_error
        got = (backward(ctx, [pairs[k]], RANGE, win, scalar=[T.G_OUTS[k]])[0], backward(ctx, [pairs[k]], RANGE, win, planes=[ups[k]])[0])
        for form, g, want in zip(("scalar", "per pixel"), got, T.model_k_grad(shape, k, window)):
            for side in range(2):
                assert np.all(np.isfinite(g[side]))
                e = float(np.abs(g[side] - want[side]).max() / np.abs(want[side]).max())
                worst = max(worst, e)
                assert e <= grad_tol, (window, k, form, "dA dB"[3 * side:3 * side + 2], e, grad_tol)
        alone.append(got)
    print("%s %s alone: worst gradient error %.3g of max|grad| (bound %.3g)" % (K.name_of(window), T.shape_id(shape), worst, grad_tol))
    pick = T.picks(n, 77)
    per = h * w + GAP
    fresh = np.full(2 * n * per + GAP, FILL32, np.float32)
    bufs = []
    try:
        dev = [(ctx.upload(a), ctx.upload(b), ctx.upload(u)) for (a, b), u in zip(pairs, ups)]
        bufs += [x for t in dev for x in t]
        out = ctx.upload(fresh)
        go = ctx.upload(np.float32([T.G_OUTS[k] for k in pick]))
        bufs += [out, go]
        ps, ms = (ssim_amd.ParamsF * n)(), (ssim_amd.GradOutF * n)()
        ga, gb = (ssim_amd.GradF * n)(), (ssim_amd.GradF * n)()
        for i, k in enumerate(pick):
            ps[i] = ssim_amd.make_params_f(w, h, dev[k][0].ptr, 1, w, dev[k][1].ptr, 1, w)
            ms[i] = ssim_amd.GradOutF(dev[k][2].ptr, 1, w)
            ga[i] = ssim_amd.GradF(out.ptr + 4 * (GAP + 2 * i * per), 1, w)
            gb[i] = ssim_amd.GradF(out.ptr + 4 * (GAP + (2 * i + 1) * per), 1, w)
        for form in (0, 1):
            assert not _device_error, "an earlier call left a device error: %r" % _device_error
            if form == 0:
                _ok(ctx.lib.rmgr_ssim_hip_enqueue_ssimf_win_grad(ctx.handle, n, ps, RANGE, _wref(win), go.ptr, ga, gb))
            else:
                out.upload(fresh)
                _ok(ctx.lib.rmgr_ssim_hip_enqueue_ssimf_win_map_grad(ctx.handle, n, ps, RANGE, _wref(win), ms, ga, gb))
            _sync(ctx)
            device.sample()
            host = out.download(np.float32, fresh.shape)
            body = host[GAP:].reshape(2 * n, per)
            assert np.all(host[:GAP] == FILL32) and np.all(body[:, h * w:] == FILL32), (window, form, "a gap between the gradient planes changed")
            got = body[:, :h * w].reshape(n, 2, h, w)
            want = np.array([alone[k][form] for k in pick], np.float32)
            bad = np.argwhere(np.any(got.view(np.uint32) != want.view(np.uint32), axis=(2, 3)))
            assert len(bad) == 0, "%s, %s upstream gradient: %d of %d gradient planes differ from the one-pair gradient; the first: pair %d (image %d), %s" % (
                K.name_of(window), ("scalar", "per-pixel")[form], len(bad), 2 * n, bad[0][0], pick[bad[0][0]], ("dA", "dB")[bad[0][1]])
    finally:
        for x in bufs:
            x.free()
