"""GPU: the 64-bit and strided-map forms of the 16-bit, float, half and multi-scale kernels, and the gradient kernels at such layouts,
held to the dense call bit for bit and to the float64 models at the bounds the families' own tests assert on dense images.

tests/test_gpu_kernel_forms.py does this for the uint8 kernels.  The four sample families each copied the strip choreography with a
64-bit form of its own (64-bit lane offsets, map offsets in elements, plain guarded map stores), selected when some pair of a launch
has a sample or map step of magnitude 2^21 or more (2^22 for the samples of the half family): a slice taken across the slices of a
volume, or a column view.  Which case reaches which instantiation:

  ssim16_strip_kernel<0, true>                 test_64_bit_forms[ssim16/10|16] (no map), test_both_sides_of_the_32_bit_limit
  ssim16_strip_kernel<1, true>                 test_64_bit_forms[ssim16/..] (map), test_a_far_apart_map_alone_..., test_mixed_batches
  ssimf_strip_kernel<0, true> / <1, true>      the same tests, [ssimf]; test_host_entry_point_on_a_column_view[ssimf]
  ssimh_strip_kernel<F16|BF16, 0, true>        test_64_bit_forms[ssimh/..] (samples 2^22 apart, no map)
  ssimh_strip_kernel<F16|BF16, 1, true>        test_64_bit_forms[ssimh/..] (samples 2^22 apart and map 2^21 apart),
                                               test_a_far_apart_map_alone_...[ssimh/..] (samples dense, map 2^21 apart: fitsh_narrow's other limit)
  msssimf_strip_kernel<true>                   test_64_bit_forms[msssimf/..], test_both_sides_..., test_mixed_batches (scale 0 only)
  every one of the nine, with offsets that     test_offsets_that_need_more_than_32_bits (columns 2^32 bytes apart; at 2^21 / 2^22 every
  do not fit 32 bits                           offset of the 64-bit forms still fits 31 bits, so the other cases cannot see a truncation)
  <0, false>, <1, false>, <2, false>           test_both_sides_of_the_32_bit_limit (steps 2^21 - 1 / 2^22 - 1: the largest 32-bit offsets),
  with a device-resident map                   test_mixed_batches (every layout narrow: the empty buffer resource of the map-less pair),
                                               test_device_resident_map_layouts (ssimStep 2 on an even width, 1 on an odd one, negative
                                               ssimStep / ssimStride, padded rows); <2, false> is every dense reference map here
  ssimf_grad / ssimh_grad / ssimw_grad /       test_gradients_at_far_apart_layouts
  msssimf_grad kernels

Layout.  One column volume per sample size and step (sample_forms_inputs.Layout): column x starts at element x * step, rows lie one
element apart.  A, B, the upstream-gradient plane and every output plane (maps, gradients) of the float family share one float32
volume, each at a row offset of its own inside the columns.  The 2-byte families keep their samples (and the half gradients) in a
uint16 volume of their own and write their float32 maps into the float volume: a map 2^21 floats apart cannot lie in columns 2^21
uint16 apart.  Everything else in a volume is filler: a NaN in the float volumes (0x7FC0, a NaN in both encodings, in the half
volumes; 0xA5A5 in the uint16 ones), a sentinel in the rows outputs are handed out from.  Every input plane is stored in four
orientations, so a view read with step -step (pointer at the last column) and / or stride -1 sees the same image and one dense
reference serves every direction.  After the launches of a test the volumes it wrote into are read back once: every output pixel
must have been written, and no other element may have changed.  test_64_bit_forms at 130 x 19 (every family, both volumes) and the
gradient test download the whole volume; the other tests read, per column, the rows in use and 4096 elements on either side of
them.  The volumes are built and uploaded once per module (about 5.2 GiB on the device and as much on the host) and freed with it.
On top of that the device holds two device-only volumes of 8 GiB (test_offsets_that_need_more_than_32_bits; three column windows
each on the host), and the host entry points stage 2 x 1 GiB while they run: the peak is what World.close() prints.

Shapes (W x H): 130 x 19 -- two 128-column strip columns, the second two pixels wide (x0 != 0, x_hi and refM clamped to W - 1, 63 lanes
with col_ok false), strips with y0 != 0 at 8-row cells, a last cell of 3 rows (ROW_LAST) -- and 3 x 300: one strip column narrower
than the halo, 38 strips of one 8-row cell each (a launch this small fits one round of wave slots, for which the planners choose
single-cell strips: every flush here carries one parked cell).  Strips of several cells, full batches of eight and the short last cell
of a tall strip are what tests/test_gpu_tall_strips.py runs.

Bounds.  None is new: ssimf_model.PX_TOL / G_TOL / GRAD_TOL, test_gpu_ssim16.PX_TOL / G_TOL, msssimf_model.VALUE_TOL / MEAN_TOL /
GRAD_TOL, ssimw_model.WGRAD_TOL; the half family is held to ssimf on the widened planes and to halfmodel's single rounding, bit for
bit.  tests/test_sample_forms_cpu.py holds the fp32 emulation of every model to these bounds on the very inputs used here.
"""
import resource
import time

import numpy as np
import pytest

import halfmodel as HM
import msssimf_model as MS
import sample_forms_inputs as IN
import ssim16_model as M16
import ssimf_model as MF
import ssimw_model as MW
import ssim_amd
from sample_forms_inputs import BIG, EDGE, EDGE_H, G_OUT, RANGE
from test_gpu_kernel_forms import SENTINEL, read_map
from test_gpu_ssim16 import G_TOL as G16_TOL, PX_TOL as PX16_TOL

pytestmark = pytest.mark.gpu

NAN32 = np.array([0x7FC0A5A5], np.uint32).view(np.float32)[0]
FILL16, NANH, OUT16 = 0xA5A5, 0x7FC0, 0xABCD
# Rows per column that output planes are handed out from.  A row is handed out once and never again: today's cases take about 10.9k
# rows of the float volume at the limit (6.4k of them the maps of test_64_bit_forms at 3 x 300) and 0.5k of the half volume; a new
# case that needs more fails with "out of output rows" until these grow.
OUT_ROWS, OUT_ROWS_H = 16384, 2048
FAR = 1 << 30                                  # floats between the columns of the device-only volumes: 4 GiB (2^31 2-byte samples)
GRAD_FILL = -777.0
MARGIN = 4096                                  # elements read back on either side of a column's rows where the whole volume is not
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def shape_id(shape):
    return "%dx%d" % (shape[1], shape[0])


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    u = UINT[got.dtype.itemsize]
    bad = np.argwhere(got.view(u) != want.view(u))
    assert len(bad) == 0, "%s: %d of %d elements differ from the dense call, first at %s: %r, want %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- the sample families ------------------------------------------------------------------------------------------------------------
class Fam(object):
    """One sample family as the cases drive it: kind "f" ssimf, "16" ssim16 at a bit depth, "h" ssimh in an encoding, "ms" msssimf at a
    configuration of scales (no maps)."""

    def __init__(self, name, kind, depth=None, enc=None, config=None):
        self.name, self.kind, self.depth, self.enc = name, kind, depth, enc
        self.config = config                     # (name, scales, weights) of sample_forms_inputs.MS_CONFIGS
        self.scales, self.weights = (config[1], config[2]) if config else (None, None)
        self.P = ssim_amd.ParamsF if kind in ("f", "ms") else ssim_amd.Params16
        self.maps = kind != "ms"

    def images(self, shape):
        if self.kind == "16":
            return IN.pair_16(shape, self.depth)
        if self.kind == "h":
            return IN.pair_h(shape, self.enc)[0]
        return IN.pair_f(shape)

    def plane(self, shape, k):
        tag = {"f": "f32", "ms": "f32", "16": "u%s" % self.depth, "h": self.enc}[self.kind]
        return "%s/%s/%s" % (tag, shape_id(shape), "ab"[k])

    def filler(self):
        return {"f": NAN32, "ms": NAN32, "16": np.uint16(FILL16), "h": np.uint16(NANH)}[self.kind]

    def make(self, w, h, ia, ib, m=None):
        f = ssim_amd.make_params_f if self.kind in ("f", "ms") else ssim_amd.make_params16
        if m is None:
            return f(w, h, *(ia + ib))
        return f(w, h, *(ia + ib), map_ptr=m[0], map_step=m[1], map_stride=m[2])

    def __repr__(self):
        return self.name


SSIMF = Fam("ssimf", "f")
FAMS = [SSIMF] + [Fam("ssim16/%d" % d, "16", depth=d) for d in IN.DEPTHS] + [Fam("ssimh/" + e, "h", enc=e) for e in HM.ENCODINGS] + \
       [Fam("msssimf/" + c[0], "ms", config=c) for c in IN.MS_CONFIGS]
MAP_FAMS = [f for f in FAMS if f.maps]
BY_FAM = pytest.mark.parametrize("fam", FAMS, ids=repr)
BY_MAP_FAM = pytest.mark.parametrize("fam", MAP_FAMS, ids=repr)
BY_SHAPE = pytest.mark.parametrize("shape", IN.SHAPES, ids=shape_id)


def launch(ctx, fam, plist):
    """One enqueue of the pairs `plist`: per pair the fp64 sum (one column), or, for msssimf, the fp64 value and the scales x 2 means."""
    n = len(plist)
    arr = (fam.P * n)(*plist)
    bufs = []
    try:
        if fam.kind == "ms":
            vals, means = ctx.upload(np.full(n, np.nan)), ctx.upload(np.full(2 * n * fam.scales, np.nan))
            bufs += [vals, means]
            ctx.enqueue_msssimf(arr, n, RANGE, vals.ptr, means.ptr, fam.scales, fam.weights)
            ctx.synchronize()
            return np.concatenate([vals.download(np.float64, (n, 1)), means.download(np.float64, (n, 2 * fam.scales))], axis=1)
        out = ctx.upload(np.full(n, np.nan))
        bufs.append(out)
        if fam.kind == "f":
            ctx.enqueue_ssimf(arr, n, RANGE, out.ptr)
        elif fam.kind == "16":
            ctx.enqueue_ssim16(arr, n, fam.depth, out.ptr)
        else:
            ctx.enqueue_ssimh(arr, n, RANGE, fam.enc, out.ptr)
        ctx.synchronize()
        return out.download(np.float64, (n, 1))
    finally:
        for b in bufs:
            b.free()


def device_value(ctx, fam, p):
    """The blocking entry point on one device-resident pair: the float32 value."""
    arr = (fam.P * 1)(p)
    if fam.kind == "f":
        return ctx.ssimf_device(arr, 1, RANGE)[0]
    if fam.kind == "16":
        return ctx.ssim16_device(arr, 1, fam.depth)[0]
    if fam.kind == "h":
        return ctx.ssimh_device(arr, 1, RANGE, fam.enc)[0]
    return ctx.msssimf_device(arr, 1, RANGE, fam.scales, fam.weights)[0]


# ---- volumes and maps ---------------------------------------------------------------------------------------------------------------
class Out(object):
    """One output plane handed out from a volume's sentinel rows, written through a view read in any direction."""

    def __init__(self, vol, h, w, flip_x, flip_y):
        self.h, self.w, self.flip_x, self.flip_y = h, w, flip_x, flip_y
        self.row0 = vol.lay.claim(h)
        off, step, stride = vol.lay.view(self.row0, h, w, flip_x, flip_y)
        self.triple = (vol.dev.ptr + vol.es * off, step, stride)
        self.plane = None                       # the plane in image orientation, once the volume was collected


class Volume(object):
    """A column volume on the device and what it must hold (self.host: outputs are folded in as they are read)."""

    def __init__(self, ctx, lay, fill, out_fill):
        self.ctx, self.lay, self.es = ctx, lay, lay.dtype.itemsize
        self.host = lay.build(fill, out_fill)
        self.dev = ctx.upload(self.host)
        self.pending = []

    def src(self, name, flip_x=False, flip_y=False):
        """(pointer, step, stride) of the input plane `name` read mirrored and / or bottom-up: always the same image."""
        h, w = self.lay.shapes[name]
        off, step, stride = self.lay.view(self.lay.rows[(name, flip_x, flip_y)], h, w, flip_x, flip_y)
        return (self.dev.ptr + self.es * off, step, stride)

    def host_view(self, name, flip_x=False, flip_y=False):
        """The same view of the HOST copy, as a numpy array with these strides."""
        h, w = self.lay.shapes[name]
        off, step, stride = self.lay.view(self.lay.rows[(name, flip_x, flip_y)], h, w, flip_x, flip_y)
        return np.lib.stride_tricks.as_strided(self.host[off:], (h, w), (self.es * stride, self.es * step), writeable=False)

    def dst(self, h, w, flip_x=False, flip_y=False):
        o = Out(self, h, w, flip_x, flip_y)
        self.pending.append(o)
        return o

    def collect(self, full=False):
        """Reads back the planes handed out since the last time and asserts that nothing else changed.  full: the whole volume in one
        download; else, per column, its rows and MARGIN elements on either side of them (the far gaps between columns are left out)."""
        lay, u = self.lay, UINT[self.es]
        if full:
            spans = [(None, 0, lay.n)]
        else:
            spans = [(x, max(0, x * lay.step - MARGIN), min(lay.n, x * lay.step + lay.end + MARGIN)) for x in range(lay.width)]
        planes = [np.empty((o.h, o.w), lay.dtype) for o in self.pending]
        bad, nbad = [], 0
        for col, lo, hi in spans:
            g = self.ctx.download(self.dev.ptr + self.es * lo, lay.dtype, (hi - lo,))
            for o, p in zip(self.pending, planes):
                for x in (range(o.w) if col is None else ([col] if col < o.w else [])):
                    at = x * lay.step + o.row0
                    p[:, x] = g[at - lo:at - lo + o.h]
                    self.host[at:at + o.h] = p[:, x]
            diff = np.flatnonzero(g.view(u) != self.host[lo:hi].view(u))
            nbad += len(diff)
            bad += [(int((i + lo) // lay.step), int((i + lo) % lay.step)) for i in diff[:8]]
            del g
        for o, p in zip(self.pending, planes):
            o.plane = np.ascontiguousarray(p[::-1 if o.flip_y else 1, ::-1 if o.flip_x else 1])
        self.pending = []
        assert nbad == 0, "%d elements outside the outputs changed; the first at (column, row) %s" % (nbad, bad[:8])

    def free(self):
        self.dev.free()
        self.host = None


def upload_at(ctx, ptr, arr):
    arr = np.ascontiguousarray(arr)
    assert ctx.lib.rmgr_ssim_hip_memcpy_h2d(ctx.handle, ptr, arr.ctypes.data, arr.nbytes) == 0


class ColumnWindows(object):
    """What a device-only volume must hold, kept for each column's rows and MARGIN elements on either side of them only: the slices
    Volume.collect(full=False) reads and writes."""

    def __init__(self, lay, fill, out_fill):
        self.win = []
        for x in range(lay.width):
            lo, hi = max(0, x * lay.step - MARGIN), min(lay.n, x * lay.step + lay.end + MARGIN)
            arr = np.full(hi - lo, fill, lay.dtype)
            arr[x * lay.step + lay.out0 - lo:x * lay.step + lay.end - lo] = out_fill
            for row0, img in lay.stored:
                if x < img.shape[1]:
                    arr[x * lay.step + row0 - lo:x * lay.step + row0 - lo + img.shape[0]] = img[:, x]
            self.win.append((lo, arr))

    def __getitem__(self, s):
        for lo, arr in self.win:
            if lo <= s.start and s.stop <= lo + len(arr):
                return arr[s.start - lo:s.stop - lo]
        raise IndexError("%r lies in no column window" % (s,))

    def __setitem__(self, s, v):
        self[s][...] = v


class FarVolume(Volume):
    """A column volume too large for a host mirror (columns 4 GiB apart): allocated on the device only; each column's window is
    uploaded, read back and compared, the gaps between them are never touched by the test."""

    def __init__(self, ctx, lay, fill, out_fill):
        self.ctx, self.lay, self.es = ctx, lay, lay.dtype.itemsize
        self.host = ColumnWindows(lay, fill, out_fill)
        self.dev = ctx.alloc(lay.n * self.es)
        for lo, arr in self.host.win:
            upload_at(ctx, self.dev.ptr + self.es * lo, arr)
        self.pending = []

    def collect(self, full=False):
        Volume.collect(self, full=False)


def map_layout(h, w, mstep=1, pad_row=0, flip_x=False, flip_y=False, lead=8):
    """A map in a buffer of its own, in the tuple test_gpu_kernel_forms.read_map takes (floats in the buffer, offset of element (0,0),
    step, stride, index of every element): elements mstep floats apart, rows padded by pad_row floats, columns and / or rows in
    reverse order, `lead` floats of sentinel before and after."""
    mrow = w * mstep + pad_row
    off = lead + ((h - 1) * mrow if flip_y else 0) + ((w - 1) * mstep if flip_x else 0)
    step, stride = (-mstep if flip_x else mstep), (-mrow if flip_y else mrow)
    idx = off + np.arange(h)[:, None] * stride + np.arange(w)[None, :] * step
    assert idx.min() >= lead and idx.max() < h * mrow + lead
    return h * mrow + 2 * lead, off, step, stride, idx


class LayMap(object):
    """A sentinel-filled device buffer holding one map laid out as map_layout() says."""

    def __init__(self, ctx, mlay):
        self.mlay = mlay
        self.buf = ctx.upload(np.full(mlay[0], SENTINEL, np.float32))
        self.triple = (self.buf.ptr + 4 * mlay[1], mlay[2], mlay[3])

    def read(self):
        try:
            return read_map(self.buf, self.mlay)
        finally:
            self.buf.free()


class Dense(object):
    """The family's default-layout call on the pair: dense device planes, a dense device-resident map, every result."""

    def __init__(self, ctx, fam, a, b):
        self.h, self.w = h, w = a.shape
        self.da, self.db = ctx.upload(a), ctx.upload(b)
        self.ia, self.ib = (self.da.ptr, 1, w), (self.db.ptr, 1, w)
        self.p = fam.make(w, h, self.ia, self.ib)
        self.res = launch(ctx, fam, [self.p])
        self.value = device_value(ctx, fam, self.p)
        self.map = None
        if fam.maps:
            m = LayMap(ctx, map_layout(h, w))
            res = launch(ctx, fam, [fam.make(w, h, self.ia, self.ib, m.triple)])
            self.map = m.read()
            assert_same_bits(res, self.res, "%s: the dense sum with and without a map" % fam)
            assert np.float32(self.res[0, 0] / (float(w) * float(h))) == self.value

    def free(self):
        self.da.free()
        self.db.free()


class World(object):
    """Everything the module builds once: the volumes and the dense references."""

    def __init__(self, ctx):
        self.ctx, self.t0 = ctx, time.time()
        self.free0 = self.min_free = ssim_amd.memory_info(ctx)[0]
        self.vols, self.dense, self.worst = {}, {}, {}
        for near in (False, True):
            f = IN.Layout(np.float32, EDGE - near, BIG[1])
            u = IN.Layout(np.uint16, EDGE - near, BIG[1])
            hv = IN.Layout(np.uint16, EDGE_H - near, BIG[1])
            for shape in IN.SHAPES:
                for fam in FAMS:
                    lay = {"f": f, "16": u, "h": hv}.get(fam.kind)
                    if lay is not None and fam.plane(shape, 0) not in lay.shapes:
                        for k, img in enumerate(fam.images(shape)):
                            lay.add(fam.plane(shape, k), img)
            f.add("gmap", IN.gmap(BIG))
            f.close(OUT_ROWS)
            u.close(8)
            hv.close(OUT_ROWS_H)
            self.vols[("f", near)] = Volume(ctx, f, NAN32, np.float32(SENTINEL))
            self.vols[("16", near)] = Volume(ctx, u, np.uint16(FILL16), np.uint16(FILL16))
            self.vols[("h", near)] = Volume(ctx, hv, np.uint16(NANH), np.uint16(OUT16))
        self.sample()

    def vol(self, fam, near=False):
        """The volume holding the family's samples: at the step that takes the 64-bit form, or (near) one below it."""
        return self.vols[({"ms": "f"}.get(fam.kind, fam.kind), near)]

    def maps(self, near=False):
        return self.vols[("f", near)]

    def far(self, fam):
        """(the device-only volume holding the family's 3 x 300 samples 4 GiB apart, the float one that takes its maps): 8 GiB each, built
        at their first use."""
        if "far" not in self.vols:
            f, u = IN.Layout(np.float32, FAR, 3), IN.Layout(np.uint16, 2 * FAR, 3)
            for other in FAMS:
                lay = {"f": f, "16": u, "h": u}.get(other.kind)
                if lay is not None:
                    for k, img in enumerate(other.images(IN.TALL)):
                        lay.add(other.plane(IN.TALL, k), img)
            f.close(4096)
            u.close(8)
            self.vols["far"] = FarVolume(self.ctx, f, NAN32, np.float32(SENTINEL))
            self.vols["far16"] = FarVolume(self.ctx, u, np.uint16(NANH), np.uint16(NANH))
        return self.vols["far" if fam.kind in ("f", "ms") else "far16"], self.vols["far"]

    def ref(self, fam, shape):
        key = (fam.name, shape)
        if key not in self.dense:
            a, b = fam.images(shape)
            d = self.dense[key] = Dense(self.ctx, fam, a, b)
            if fam.kind == "h":                  # the float32 path on the widened planes, which the half family is held to
                fa, fb = IN.pair_h(shape, fam.enc)[1]
                d.wide = Dense(self.ctx, SSIMF, fa, fb)
                d.wide.free()
        return self.dense[key]

    def sample(self):
        self.min_free = min(self.min_free, ssim_amd.memory_info(self.ctx)[0])

    def close(self):
        self.sample()
        for d in self.dense.values():
            d.free()
        for v in self.vols.values():
            v.free()
        self.ctx.trim()
        print("\nsample forms: module wall time %.1f s; peak device memory in use by the module %.2f GiB; peak host RSS %.2f GiB" % (
            time.time() - self.t0, (self.free0 - self.min_free) / 2.0 ** 30, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2.0 ** 20))


@pytest.fixture(scope="module")
def world(gpu_ctx):
    w = World(gpu_ctx)
    yield w
    w.close()


# ---- the second assertion: the float64 definition -----------------------------------------------------------------------------------
def hold(world, fam, shape, res, m, form):
    """Holds one result (a row of launch() and the map, or None) to the family's float64 model at the bounds of its own GPU test; the
    half family to ssimf on the widened planes, bit for bit.  Keeps the worst figures per (family, form) for report()."""
    h, w = shape
    px = g = 0.0
    if fam.kind in ("f", "16"):
        gv, gm = IN.model(("ssimf", shape)) if fam.kind == "f" else IN.model(("ssim16", shape, fam.depth))
        bound = (MF.PX_TOL, MF.G_TOL) if fam.kind == "f" else (PX16_TOL, G16_TOL)
        g = abs(float(np.float32(res[0] / (float(w) * float(h)))) - gv)
        if m is not None:
            px = float(np.abs(m.astype(np.float64) - gm).max())
    elif fam.kind == "h":
        wide = world.ref(fam, shape).wide
        bound = (0, 0)
        g = int(res.view(np.uint64)[0] != wide.res.view(np.uint64)[0, 0])
        if m is not None:
            px = int(m.size) if not HM.same_f32(m, wide.map) else 0
    else:
        gv, gm = IN.model(("msssimf", shape, fam.config[0]))
        bound = (MS.MEAN_TOL, MS.VALUE_TOL)
        g = abs(float(res[0]) - gv)
        px = float(np.abs(res[1:].reshape(fam.scales, 2) - gm).max())
    key = (fam.name, form)
    wp, wg = world.worst.get(key, (0, 0, None))[:2]
    world.worst[key] = (max(wp, px), max(wg, g), bound)
    assert px <= bound[0], (fam, form, "per-pixel error (msssimf: per-scale mean)", px, bound[0])
    assert g <= bound[1], (fam, form, "global error", g, bound[1])


def report(world, title):
    print("\n%s: worst error per family and form (bound); ssimh: pixels / sums that differ from ssimf on the widened planes" % title)
    for (name, form), (px, g, bound) in sorted(world.worst.items()):
        print("  %-18s %-44s per pixel %-22s global %.3g (%.3g)" % (name, form, "%.3g (%.3g)" % (px, bound[0]), g, bound[1]))
    world.worst.clear()


def check_pair(world, fam, shape, res, out, what, form):
    """Both assertions on one pair of a launch: res its row of launch(), out its map (an Out or LayMap already read, or None)."""
    ref = world.ref(fam, shape)
    assert_same_bits(res, ref.res[0], what + ": sum")
    m = None
    if out is not None:
        m = out.plane if isinstance(out, Out) else out
        assert_same_bits(m, ref.map, what + ": map")
    hold(world, fam, shape, res, m, form)


# reading directions: (name, (flip_x, flip_y) of A, of B, of the map)
DIRECTIONS = (("+x +y", (False, False), (False, False), (False, False)),
              ("mirrored", (True, False), (True, False), (True, False)),
              ("bottom-up", (False, True), (False, True), (False, True)),
              ("A mirrored, B bottom-up, map both", (True, False), (False, True), (True, True)))


# ---- 1. the 64-bit forms ------------------------------------------------------------------------------------------------------------
@BY_SHAPE
@BY_FAM
def test_64_bit_forms(world, fam, shape):
    """Samples 2^21 apart (2^22 for the half family), and with them a map 2^21 floats apart, in every reading direction, without a map
    and with one: every launch takes the family's 64-bit form.  In one direction A and B differ in the sign of their step (refA !=
    refB).  The blocking device entry point on the same view gives the dense value."""
    ctx, (h, w) = world.ctx, shape
    vol, mvol, ref = world.vol(fam), world.maps(), world.ref(fam, shape)
    done = []
    for dname, fa, fb, fm in DIRECTIONS:
        ia, ib = vol.src(fam.plane(shape, 0), *fa), vol.src(fam.plane(shape, 1), *fb)
        assert abs(ia[1]) >= (EDGE_H if fam.kind == "h" else EDGE)
        done.append((dname, "no map", launch(ctx, fam, [fam.make(w, h, ia, ib)])[0], None))
        if fam.maps:
            o = mvol.dst(h, w, *fm)
            done.append((dname, "map", launch(ctx, fam, [fam.make(w, h, ia, ib, o.triple)])[0], o))
    v = device_value(ctx, fam, fam.make(w, h, vol.src(fam.plane(shape, 0), True, True), vol.src(fam.plane(shape, 1))))
    assert v.tobytes() == ref.value.tobytes(), (fam, float(v), float(ref.value))
    mvol.collect(full=shape == BIG)                  # the whole volume once per family; 3 x 300: the rows in use and their margins
    if vol is not mvol:
        vol.collect(full=shape == BIG)
    for dname, mname, res, o in done:
        check_pair(world, fam, shape, res, o, "%s %s, 64-bit form, %s, %s" % (fam, shape_id(shape), dname, mname), "64-bit, " + mname)
    world.sample()
    report(world, "64-bit forms, %s" % shape_id(shape))


# ---- 2. a map-only trigger ----------------------------------------------------------------------------------------------------------
@BY_SHAPE
@BY_MAP_FAM
def test_a_far_apart_map_alone_selects_the_64_bit_form(world, fam, shape):
    """Dense images with a map 2^21 floats apart, forwards and in the negative direction.  For the half family this is the second limit
    of fitsh_narrow(): the samples would fit."""
    ctx, (h, w) = world.ctx, shape
    mvol, ref = world.maps(), world.ref(fam, shape)
    for dname, fm in (("+x +y", (False, False)), ("mirrored and bottom-up", (True, True))):
        o = mvol.dst(h, w, *fm)
        res = launch(ctx, fam, [fam.make(w, h, ref.ia, ref.ib, o.triple)])[0]
        mvol.collect()                                   # after each launch: the next one starts from a volume known to be intact
        check_pair(world, fam, shape, res, o, "%s %s, dense images, far-apart map %s" % (fam, shape_id(shape), dname), "64-bit, map-only trigger")
    report(world, "map-only trigger, %s" % shape_id(shape))


# ---- 3. both sides of the edge ------------------------------------------------------------------------------------------------------
@BY_FAM
def test_both_sides_of_the_32_bit_limit(world, fam):
    """The same pixels one step below the limit (2^21 - 1; 2^22 - 1 for half samples, with the map at 2^21 - 1): the 32-bit forms at
    their largest lane offsets, 143 columns x step x sample size, and map offsets just below the 0x80000000 that stands for "store
    nothing"; and at the limit: the 64-bit form.  With a map at that step read forwards and in the negative direction, and without.
    Both sides give the bits of the dense call."""
    ctx, shape, (h, w) = world.ctx, BIG, BIG
    done = []
    for near in (True, False):
        vol, mvol = world.vol(fam, near), world.maps(near)
        side = "below the limit" if near else "at the limit"
        for dname, fa, fb, fm in (DIRECTIONS[0], DIRECTIONS[3], DIRECTIONS[1]):
            ia, ib = vol.src(fam.plane(shape, 0), *fa), vol.src(fam.plane(shape, 1), *fb)
            assert (abs(ia[1]) < (EDGE_H if fam.kind == "h" else EDGE)) == near
            done.append((side, dname + ", no map", launch(ctx, fam, [fam.make(w, h, ia, ib)])[0], None))
            if fam.maps:
                o = mvol.dst(h, w, *fm)
                assert (abs(o.triple[1]) < EDGE) == near
                done.append((side, dname + ", map", launch(ctx, fam, [fam.make(w, h, ia, ib, o.triple)])[0], o))
        mvol.collect()
        if vol is not mvol:
            vol.collect()
    for side, dname, res, o in done:
        check_pair(world, fam, shape, res, o, "%s, %s, %s" % (fam, side, dname), side)
    report(world, "both sides of the 32-bit limit, 130x19")


@BY_FAM
def test_offsets_that_need_more_than_32_bits(world, fam):
    """At the steps above no lane offset of the 64-bit forms needs more than 31 bits (129 columns x 2^21 x 4 B is about 1.08e9), so an
    instantiation that truncated (xg - refA) * step * 4, or the map offset, to 32 bits would pass them.  Here 3 x 300 pixels lie 2^30
    floats apart (2^31 half or uint16 samples), and the map with them: column 1 is 2^32 bytes and column 2 is 2^33 bytes from column 0,
    so a truncated offset lands on column 0.  The volumes live on the device only (8 GiB each, three column windows uploaded).  Forwards,
    and with A mirrored, B bottom-up and the map both; without a map and with one."""
    ctx, shape, (h, w) = world.ctx, IN.TALL, IN.TALL
    vol, mvol = world.far(fam)
    done = []
    for dname, fa, fb, fm in (DIRECTIONS[0], DIRECTIONS[3]):
        ia, ib = vol.src(fam.plane(shape, 0), *fa), vol.src(fam.plane(shape, 1), *fb)
        assert abs(ia[1]) * vol.es == 1 << 32
        done.append((dname + ", no map", launch(ctx, fam, [fam.make(w, h, ia, ib)])[0], None))
        if fam.maps:
            o = mvol.dst(h, w, *fm)
            done.append((dname + ", map", launch(ctx, fam, [fam.make(w, h, ia, ib, o.triple)])[0], o))
    mvol.collect()
    if vol is not mvol:
        vol.collect()
    for dname, res, o in done:
        check_pair(world, fam, shape, res, o, "%s, columns 4 GiB apart, %s" % (fam, dname), "64-bit, columns 4 GiB apart")
    world.sample()
    report(world, "offsets beyond 32 bits, 3x300")


# ---- 4. mixed batches ---------------------------------------------------------------------------------------------------------------
def interleaved(ctx, fam, img, step):
    """The plane as the last channel of a `step`-channel interleaved buffer: (device buffer, (pointer, step, stride))."""
    h, w = img.shape
    host = np.full((h, w, step), fam.filler(), img.dtype)
    host[:, :, step - 1] = img
    d = ctx.upload(host)
    return d, (d.ptr + img.dtype.itemsize * (step - 1), step, w * step)


@BY_FAM
def test_mixed_batches(world, fam):
    """Three pairs of one size in one enqueue: a dense pair with a dense map, a pair in another layout with a map in that layout, and a
    dense pair without a map (msssimf: no maps).  With the middle pair in the column volume one failing pair switches the whole launch to
    the 64-bit form, where the map-less pair meets the has_map guard; with the middle pair at step 3 every layout is narrow and the
    map-less pair's buffer resource is empty (map_records = 0).  Each pair has the bits it has alone; no buffer is touched outside
    its map."""
    ctx, shape, (h, w) = world.ctx, BIG, BIG
    vol, mvol, ref = world.vol(fam), world.maps(), world.ref(fam, shape)
    a, b = fam.images(shape)
    swapped = fam.make(w, h, ref.ib, ref.ia)                                     # the third pair: (B, A), dense, no map
    alone = launch(ctx, fam, [swapped])[0]
    keep = []
    try:
        da3, ia3 = interleaved(ctx, fam, a, 3)
        db3, ib3 = interleaved(ctx, fam, b, 3)
        keep += [da3, db3]
        for form in ("64-bit", "32-bit"):
            m0 = LayMap(ctx, map_layout(h, w)) if fam.maps else None
            if form == "64-bit":
                ia, ib = vol.src(fam.plane(shape, 0), True, False), vol.src(fam.plane(shape, 1))
                m1 = mvol.dst(h, w) if fam.maps else None
            else:
                ia, ib = ia3, ib3
                m1 = LayMap(ctx, map_layout(h, w, mstep=3, pad_row=2)) if fam.maps else None
            plist = [fam.make(w, h, ref.ia, ref.ib, m0.triple if m0 else None), fam.make(w, h, ia, ib, m1.triple if m1 else None), swapped]
            res = launch(ctx, fam, plist)
            what = "%s, mixed batch, %s" % (fam, form)
            if form == "64-bit":
                mvol.collect()
                if vol is not mvol:
                    vol.collect()
            check_pair(world, fam, shape, res[0], m0.read() if m0 else None, what + ", dense pair with a map", "mixed batch, " + form)
            check_pair(world, fam, shape, res[1], (m1 if isinstance(m1, Out) else m1.read()) if m1 else None, what + ", middle pair",
                       "mixed batch, " + form)
            assert_same_bits(res[2], alone, what + ", pair without a map")
    finally:
        for d in keep:
            d.free()
    report(world, "mixed batches, 130x19")


# ---- 5. device-resident map layouts in the 32-bit forms ----------------------------------------------------------------------------
MAP_LAYOUTS = (("ssimStep 4, even width", 130, dict(mstep=4)),
               ("ssimStep 2, even width", 130, dict(mstep=2)),
               ("ssimStep 1, odd width, padded rows", 129, dict(pad_row=3)),
               ("ssimStep -1", 130, dict(flip_x=True)),
               ("ssimStride < 0, padded rows", 130, dict(flip_y=True, pad_row=6)),
               ("ssimStep -3, ssimStride < 0, padded rows, odd width", 129, dict(mstep=3, flip_x=True, flip_y=True, pad_row=5)),
               ("ssimStep 2, ssimStride < 0, even width", 130, dict(mstep=2, flip_y=True)))


@BY_MAP_FAM
def test_device_resident_map_layouts(world, fam):
    """The map in device memory at layouts the host entry points never pass on (they stage a dense map): form MAP == 1 on an even width
    because ssimStep is 4 or 2, on an odd width at ssimStep 1 with padded rows, negative ssimStep (refM on the strip's right end) and
    ssimStride, padded rows; MAP == 2 is the dense reference of the even width, and once more bottom-up with padded rows.  130 x 19 and
    its first 129 columns (sample_forms_inputs.crop; the CPU test emulates both).  Each map equals the dense map of that width bit for
    bit, with sentinels around and between its elements, and the dense map meets the model."""
    ctx, (h, _) = world.ctx, BIG
    for w in (130, 129):
        ca, cb = IN.crop(fam.images(BIG), w)
        d = Dense(ctx, fam, ca, cb)
        try:
            if fam.kind == "h":
                wide = Dense(ctx, SSIMF, HM.widen(ca, fam.enc), HM.widen(cb, fam.enc))
                wide.free()
                assert HM.same_f32(d.map, wide.map) and d.res.tobytes() == wide.res.tobytes(), (fam, w)
            else:
                gv, gm = MF.ssim(ca, cb, RANGE) if fam.kind == "f" else M16.ssim(ca.astype(np.int64), cb.astype(np.int64), fam.depth)
                bound = (MF.PX_TOL, MF.G_TOL) if fam.kind == "f" else (PX16_TOL, G16_TOL)
                px, g = float(np.abs(d.map.astype(np.float64) - gm).max()), abs(float(d.value) - gv)
                assert px <= bound[0] and g <= bound[1], (fam, w, px, g)
            for name, lw, kw in MAP_LAYOUTS:
                if lw != w:
                    continue
                m = LayMap(ctx, map_layout(h, w, **kw))
                res = launch(ctx, fam, [fam.make(w, h, d.ia, d.ib, m.triple)])
                got = m.read()
                assert_same_bits(res, d.res, "%s, %s: sum" % (fam, name))
                assert_same_bits(got, d.map, "%s, %s: map" % (fam, name))
        finally:
            d.free()


# ---- 6. gradients at these layouts --------------------------------------------------------------------------------------------------
class GradKind(object):
    """One gradient entry point as the case drives it."""

    def __init__(self, name, fam, entry):
        self.name, self.fam, self.entry = name, fam, entry
        self.half = fam.kind == "h"
        self.G = ssim_amd.GradH if self.half else ssim_amd.GradF

    def g_out(self, shape):
        return IN.g_out_h(*shape) if self.half else G_OUT

    def run(self, ctx, p, shape, ga, gb, gmap=None):
        """One enqueue on the pair `p`: gradients into the planes ga / gb ((pointer, step, stride) or None)."""
        fam = self.fam
        arr = (fam.P * 1)(p)
        arrs = [None if t is None else (self.G * 1)(self.G(*t)) for t in (ga, gb)]
        bufs = [ctx.upload(np.float32([self.g_out(shape)]))]
        try:
            if self.entry == "ssimf_grad":
                ctx.enqueue_ssimf_grad(arr, 1, RANGE, bufs[0].ptr, arrs[0], arrs[1])
            elif self.entry == "ssimh_grad":
                ctx.enqueue_ssimh_grad(arr, 1, RANGE, fam.enc, bufs[0].ptr, arrs[0], arrs[1])
            elif self.entry == "ssimf_map_grad":
                ctx.enqueue_ssimf_map_grad(arr, 1, RANGE, (ssim_amd.GradOutF * 1)(ssim_amd.GradOutF(*gmap)), arrs[0], arrs[1])
            else:
                vals, means = ctx.alloc(8), ctx.alloc(16 * fam.scales)
                bufs += [vals, means]
                ctx.enqueue_msssimf(arr, 1, RANGE, vals.ptr, means.ptr, fam.scales, fam.weights)
                ctx.enqueue_msssimf_grad(arr, 1, RANGE, means.ptr, bufs[0].ptr, arrs[0], arrs[1], fam.scales, fam.weights)
            ctx.synchronize()
        finally:
            for x in bufs:
                x.free()

    def __repr__(self):
        return self.name


GRAD_KINDS = [GradKind("ssimf_grad", SSIMF, "ssimf_grad")] + \
             [GradKind("ssimh_grad/" + f.enc, f, "ssimh_grad") for f in FAMS if f.kind == "h"] + \
             [GradKind("ssimf_map_grad", SSIMF, "ssimf_map_grad")] + \
             [GradKind("msssimf_grad/" + f.config[0], f, "msssimf_grad") for f in FAMS if f.kind == "ms"]
# (name, (flip_x, flip_y) of A, B, the upstream-gradient plane, dLoss/dA, dLoss/dB)
GRAD_DIRECTIONS = (("+x +y", (False, False), (False, False), (False, False), (False, False), (False, False)),
                   ("mirrored and bottom-up", (True, True), (True, True), (True, True), (True, True), (True, True)),
                   ("mixed signs", (True, False), (False, True), (True, False), (False, True), (True, False)))


def hold_grad(kind, shape, got, which, dense32):
    """The float64 definition of one gradient plane (which: 0 dLoss/dA, 1 dLoss/dB); the half family: halfmodel's single rounding of the
    float32 path's gradient of the widened planes (dense32), bit for bit.  Returns (error, bound)."""
    if kind.half:
        want = HM.round_to(dense32[which], kind.fam.enc)
        assert HM.same(got, want, kind.fam.enc), (kind, "dA dB"[3 * which:3 * which + 2], "differs from the rounded float32 gradient")
        assert (got & 0x7FFF).max() > 0
        return 0, 0
    if kind.entry == "ssimf_grad":
        want, bound = IN.model(("ssimf_grad", shape))[which], MF.GRAD_TOL
    elif kind.entry == "ssimf_map_grad":
        want, bound = IN.model(("ssimw", shape))[which], MW.WGRAD_TOL
    else:
        want, bound = IN.model(("msssimf_grad", shape, kind.fam.config[0]))[which], MS.GRAD_TOL
    assert np.all(np.isfinite(got))
    e = float(np.abs(got - want).max() / np.abs(want).max())
    assert e <= bound, (kind, "dA dB"[3 * which:3 * which + 2], e, bound)
    return e, bound


@pytest.mark.parametrize("kind", GRAD_KINDS, ids=repr)
def test_gradients_at_far_apart_layouts(world, kind):
    """rmgr_ssim_hip_enqueue_ssimf_grad, _ssimh_grad, _ssimf_map_grad and _msssimf_grad with the inputs, the gradient planes and (map
    gradient) the upstream-gradient plane 2^21 elements apart (2^22 for half samples), in three combinations of signs; dLoss/dA alone,
    dLoss/dB alone and both.  Every plane equals the dense-layout call bit for bit and meets the model."""
    ctx, shape, (h, w) = world.ctx, BIG, BIG
    fam = kind.fam
    vol, fvol, ref = world.vol(fam), world.maps(), world.ref(fam, shape)
    gvol = vol if kind.half else fvol                       # where the gradient planes live: in the samples' type
    dt, fill = (np.uint16, np.uint16(OUT16)) if kind.half else (np.float32, np.float32(GRAD_FILL))
    keep = []
    try:
        # the dense-layout call: both gradients into dense planes
        dg = [ctx.upload(np.full((h, w), fill, dt)) for _ in range(2)]
        keep += dg
        dgm = None
        if kind.entry == "ssimf_map_grad":
            dgm = ctx.upload(IN.gmap(shape))
            keep.append(dgm)
        kind.run(ctx, ref.p, shape, (dg[0].ptr, 1, w), (dg[1].ptr, 1, w), (dgm.ptr, 1, w) if dgm else None)
        dense = [d.download(dt, (h, w)) for d in dg]
        dense32 = None
        if kind.half:                                        # the float32 path's gradient of the widened planes, same gOut
            fa, fb = IN.pair_h(shape, fam.enc)[1]
            wide = Dense(ctx, SSIMF, fa, fb)
            fg = [ctx.upload(np.full((h, w), np.float32(GRAD_FILL))) for _ in range(2)]
            keep += fg + [wide.da, wide.db]
            arrs = [(ssim_amd.GradF * 1)(ssim_amd.GradF(x.ptr, 1, w)) for x in fg]
            go = ctx.upload(np.float32([kind.g_out(shape)]))
            keep.append(go)
            ctx.enqueue_ssimf_grad((ssim_amd.ParamsF * 1)(wide.p), 1, RANGE, go.ptr, arrs[0], arrs[1])
            ctx.synchronize()
            dense32 = [x.download(np.float32, (h, w)) for x in fg]
        worst = 0
        for which in range(2):
            e, bound = hold_grad(kind, shape, dense[which], which, dense32)
            worst = max(worst, e)
        done = []
        for dname, fa_, fb_, fm_, fga, fgb in GRAD_DIRECTIONS:
            ia, ib = vol.src(fam.plane(shape, 0), *fa_), vol.src(fam.plane(shape, 1), *fb_)
            gm = fvol.src("gmap", *fm_) if kind.entry == "ssimf_map_grad" else None
            p = fam.make(w, h, ia, ib)
            for want_a, want_b in ((True, True), (True, False), (False, True)):
                oa = gvol.dst(h, w, *fga) if want_a else None
                ob = gvol.dst(h, w, *fgb) if want_b else None
                kind.run(ctx, p, shape, oa.triple if oa else None, ob.triple if ob else None, gm)
                done.append((dname, oa, ob))
        gvol.collect(full=True)
        for dname, oa, ob in done:
            for which, o in enumerate((oa, ob)):
                if o is not None:
                    what = "%s, %s, %s%s" % (kind, dname, "dLoss/dA" if which == 0 else "dLoss/dB", "" if oa and ob else " alone")
                    assert_same_bits(o.plane, dense[which], what)
    finally:
        for d in keep:
            d.free()
    world.sample()
    print("\n%s at far-apart layouts, 130x19: %d planes bit-identical to the dense call; worst error %.3g of max|grad| (bound %.3g)" % (
        kind, sum((oa is not None) + (ob is not None) for _, oa, ob in done), worst, bound))


# ---- 7. the host entry points on the same view -------------------------------------------------------------------------------------
@BY_MAP_FAM
def test_host_entry_point_on_a_column_view(world, fam):
    """compute_ssimf / compute_ssim16 / compute_ssimh on numpy views of the HOST copy of the volume, A mirrored (a negative step), with a
    map.  This exercises the staging gather of the host entry points -- each image's whole sample extent, about 1 GiB, is copied to the
    device and the kernel reads it at the same far-apart step, writing a dense staged map -- not another kernel form.  Value and map
    have the bits of the dense call."""
    ctx, shape = world.ctx, BIG
    vol, ref = world.vol(fam), world.ref(fam, shape)
    a, b = vol.host_view(fam.plane(shape, 0), True, False), vol.host_view(fam.plane(shape, 1))
    assert np.array_equal(a, fam.images(shape)[0]) and a.strides[1] < 0
    if fam.kind == "f":
        v, m = ssim_amd.compute_ssimf(a, b, RANGE, want_map=True, ctx=ctx)
    elif fam.kind == "16":
        v, m = ssim_amd.compute_ssim16(a, b, fam.depth, want_map=True, ctx=ctx)
    else:
        (ha, st), (hb, _) = HM.host_array(a, fam.enc), HM.host_array(b, fam.enc)
        v, m = ssim_amd.compute_ssimh(ha, hb, RANGE, sample_type=st, want_map=True, ctx=ctx)
    world.sample()
    ctx.trim()
    assert v.tobytes() == ref.value.tobytes(), (fam, float(v), float(ref.value))
    assert_same_bits(m, ref.map, "%s, host entry point on a column view" % fam)
