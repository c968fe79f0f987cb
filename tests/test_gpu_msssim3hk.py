"""GPU: multi-scale SSIM of float16 / bfloat16 volumes under a caller-chosen window and its gradient (rmgr_ssim_hip_*_msssim3h_win*,
msssim3hk_kernels.hip) against the float32 windowed entries, BIT FOR BIT.  Sizes are W x H x D; arrays are (D, H, W); 16-bit samples travel
as uint16 bit patterns.

The contract (include/rmgr/ssim-hip.h): the value and both means of every scale have the bits rmgr_ssim_hip_enqueue_msssim3f_win gives on
the widened volumes under the same window; a gradient voxel is the float32 value _enqueue_msssim3f_win_grad would store at scale 0, rounded
once, to nearest-even, into the inputs' encoding.  So every comparison here runs the float32 entry in the same test on
halfmodel.widen(samples) and compares bits -- gradients against halfmodel.round_to(float32 gradient) -- and there is no tolerance.  No
float64 model runs here: tests/test_gpu_msssim3k.py holds the float32 entries to it.

Every 16-bit call keeps its inputs, its gradient volumes, its values and its means in buffers with sentinel gaps (test_gpu_ssim3h.Arena);
after every call the gaps and every element of a strided buffer outside the volumes are asserted untouched.
"""
import ctypes
import errno

import numpy as np
import pytest

import halfmodel as HM
import msssim3k_inputs as IN3
import msssim3k_model as MK
import ssim3h_inputs as IN
import ssim_amd
from test_gpu_msssim3h import same64, uniform, upload_inputs
from test_gpu_msssim3h import run as run_fixed
from test_gpu_msssim3k import PER_RADIUS
from test_gpu_msssim3k import run as run_f32
from test_gpu_ssim3h import LAYOUTS, MAX16, SENT, Arena, Device, call
from test_gpu_ssim3k import mk

pytestmark = pytest.mark.gpu

ENC = pytest.mark.parametrize("enc", HM.ENCODINGS)
BY_WINDOW = pytest.mark.parametrize("window", MK.WINDOWS, ids=MK.name_of)
BY_RADIUS = pytest.mark.parametrize("window", PER_RADIUS, ids=MK.name_of)
BOX3, G9 = IN3.ODD_WINDOWS
ENGINE = (11, 1.5, "gaussian")


@pytest.fixture(scope="module")
def device(gpu_ctx):
    d = Device(gpu_ctx)
    yield d
    d.close()


def run(device, enc, pairs, r, window, scales=5, weights=None, g_out=None, want=(True, True), lin="dense", lout="dense"):
    """Forward (values, means) and -- g_out given -- backward of `pairs` (uint16 bit patterns) under `window` (a model window) in ONE
    enqueue each, device-resident.  Returns (values float64 (n,), means float64 (n, scales, 2), [(dA or None, dB or None)] as uint16)."""
    ctx, win = device.ctx, mk(window)
    arenas = []
    try:
        ins = upload_inputs(device, pairs, lin)
        arenas.append(ins)
        n = len(pairs)
        d, h, w = ins.items[0][3].shape
        out = Arena(np.float64)
        out.add((1, 1, n))
        out.add((1, 1, 2 * n * scales))
        arenas.append(out.upload(ctx))
        ps = (ssim_amd.Params3H * n)()
        for i in range(n):
            (pa, sa), (pb, sb) = ins.at(2 * i), ins.at(2 * i + 1)
            ps[i] = ssim_amd.make_params3h(w, h, d, pa, sa, pb, sb)
        call(ctx.enqueue_msssim3h, ps, n, r, enc, out.at(0)[0], out.at(1)[0], scales, weights, win)
        gar, idx = Arena(np.uint16), [[], []]
        if g_out is not None:
            up = Arena(np.float32)
            up.add((1, 1, n), "dense", np.asarray(g_out, np.float32).reshape(1, 1, n))
            arenas.append(up.upload(ctx))
            for k in range(2):
                if want[k]:
                    idx[k] = [gar.add((d, h, w), lout) for _ in range(n)]
            arenas.append(gar.upload(ctx))
            arrs = [None, None]
            for k in range(2):
                if want[k]:
                    arrs[k] = (ssim_amd.Grad3H * n)()
                    for i in range(n):
                        p, s = gar.at(idx[k][i])
                        arrs[k][i] = ssim_amd.Grad3H(p, *s)
            call(ctx.enqueue_msssim3h_grad, ps, n, r, enc, out.at(1)[0], up.at(0)[0], arrs[0], arrs[1], scales, weights, win)
        call(ctx.synchronize)
        device.sample()
        v, m = out.results(written=True)
        grads = []
        if g_out is not None:
            got = gar.results()
            grads = [(got[idx[0][i]] if want[0] else None, got[idx[1][i]] if want[1] else None) for i in range(n)]
            up.results()
        ins.results()                                      # the inputs and everything around them are unchanged
        return v.reshape(n), m.reshape(n, scales, 2), grads
    finally:
        for a in arenas:
            a.free()


def reference(device, enc, pairs, r, window, scales, weights, g_out=None):
    """msssim3f_win on the widened volumes: (values, means, [(dA, dB) rounded once into the encoding], the float32 gradients)."""
    v, m, gr = run_f32(device.ctx, [(HM.widen(a, enc), HM.widen(b, enc)) for a, b in pairs], r, window, scales, weights, g_out)
    return v, m, [(HM.round_to(ga, enc), HM.round_to(gb, enc)) for ga, gb in gr], gr


def check_against_float32(device, enc, pairs, r, window, scales, weights, g_out, what, one_gradient=False, **kw):
    """One call of the 16-bit entries against the same call of the float32 entries on the widened volumes."""
    got = run(device, enc, pairs, r, window, scales, weights, g_out, **kw)
    ref = reference(device, enc, pairs, r, window, scales, weights, g_out)
    assert same64(got[0], ref[0]) and same64(got[1], ref[1]), (what, got[0], ref[0])
    assert len(got[2]) == len(ref[2]) == (len(pairs) if g_out is not None else 0)
    for (ga, gb), (fa, fb) in zip(got[2], ref[2]):
        assert ga.dtype == np.uint16 and HM.same(ga, fa, enc) and HM.same(gb, fb, enc), what
    if one_gradient:
        only_a = run(device, enc, pairs, r, window, scales, weights, g_out, want=(True, False), **kw)
        only_b = run(device, enc, pairs, r, window, scales, weights, g_out, want=(False, True), **kw)
        for i in range(len(pairs)):
            assert only_a[2][i][1] is None and only_b[2][i][0] is None
            assert HM.same(only_a[2][i][0], ref[2][i][0], enc) and HM.same(only_b[2][i][1], ref[2][i][1], enc), what
    return got, ref


def voxel_scale(size):
    """A dLoss/dMS of the order of the voxel count: the gradient of a mean is of order 1 / (W H D), which float16 would flush."""
    return -0.75 * float(size[0] * size[1] * size[2])


def odd_pair16(index, enc):
    a, b = IN3.odd_pair(index)
    return HM.round_to(a, enc), HM.round_to(b, enc)


# ---- the seven windows on the odd sizes -------------------------------------------------------------------------------------------------

@ENC
@BY_WINDOW
def test_value_means_and_gradients_have_the_float32_bits_on_the_odd_sizes(device, enc, window):
    """The eight seeded odd sizes at 8 uniform scales under every window (the 11-tap ones run msssim3h_kernels.hip with the window's taps);
    the two smallest also at one scale (the ssim form and kMsLast at scale 0) and with a zero weight at scale 0."""
    for i, size in enumerate(IN3.ODD_SIZES):
        pair = odd_pair16(i, enc)
        sets = [(IN3.ODD_SCALES, uniform(IN3.ODD_SCALES))] + ([(1, (1.0,)), (3, (0.0, 0.5, 0.5))] if i in (2, 5) else [])
        for scales, weights in sets:
            got, ref = check_against_float32(device, enc, [pair], 1.0, window, scales, weights, [voxel_scale(size)], (size, scales),
                                             one_gradient=i in (2, 7))
            if size != (1, 1, 1):
                assert np.abs(ref[3][0][0]).max() > 0 and np.any(got[2][0][0] & 0x7FFF), (size, scales)


# ---- a batch, and the host entry --------------------------------------------------------------------------------------------------------

@ENC
@pytest.mark.parametrize("window", [BOX3, (7, 1.5, "gaussian")], ids=MK.name_of)
def test_a_batch_and_the_host_and_device_entries(device, enc, window):
    size = (33, 20, 13)
    win = mk(window)
    pairs = [IN.random_pair(size, 40 + i, enc) for i in range(5)]
    g = [x * float(33 * 20 * 13) for x in (-0.75, 1.5, 0.0, 1.0, -2.0)]
    got, ref = check_against_float32(device, enc, pairs, 1.0, window, 4, uniform(4), g, "a batch of five")
    for t in got[2][2]:
        assert not np.any(t), "gOut = 0: a gradient voxel is not +0"
    alone = run(device, enc, [pairs[3]], 1.0, window, 4, uniform(4), [g[3]])
    assert same64(alone[0], got[0][3:4]) and HM.same(alone[2][0][0], got[2][3][0], enc) and HM.same(alone[2][0][1], got[2][3][1], enc)
    again = run(device, enc, pairs, 1.0, window, 4, uniform(4), g)
    assert same64(again[0], got[0]) and all(HM.same(x, y, enc) for p, q in zip(again[2], got[2]) for x, y in zip(p, q))
    hosts = [(HM.host_array(a, enc)[0], HM.host_array(b, enc)[0]) for a, b in pairs]
    st = HM.host_array(pairs[0][0], enc)[1]
    for ctx in (None, device.ctx):
        vs, ms = call(ssim_amd.compute_msssim3h_batch, hosts, 1.0, st, 4, uniform(4), True, ctx, win)
        assert vs.tobytes() == got[0].astype(np.float32).tobytes() and same64(ms, got[1])
    hv, hm = call(ssim_amd.compute_msssim3h, hosts[1][0], hosts[1][1], 1.0, st, 4, uniform(4), True, None, win)
    assert np.float32(hv).tobytes() == np.float32(got[0][1]).tobytes() and same64(hm, got[1][1])
    ins = upload_inputs(device, pairs[:2])
    try:
        ps = (ssim_amd.Params3H * 2)()
        for i in range(2):
            ps[i] = ssim_amd.make_params3h(size[0], size[1], size[2], ins.at(2 * i)[0], ins.at(2 * i)[1], ins.at(2 * i + 1)[0], ins.at(2 * i + 1)[1])
        dv, dm = call(device.ctx.msssim3h_device, ps, 2, 1.0, enc, 4, uniform(4), True, win)
        assert dv.tobytes() == got[0][:2].astype(np.float32).tobytes() and same64(dm, got[1][:2])
    finally:
        ins.free()


# ---- the default window is msssim3h -----------------------------------------------------------------------------------------------------

@ENC
def test_null_and_the_engines_window_give_the_bits_of_msssim3h(device, enc):
    ctx, lib = device.ctx, device.ctx.lib
    size = (33, 20, 13)
    w, h, d = size
    pairs = [IN.random_pair(size, 5, enc), IN.random_pair(size, 6, enc)]
    g = [voxel_scale(size), 0.5 * w * h * d]
    code = ssim_amd.sample_type_code(enc)
    for scales, wts in ((5, None), (3, (0.2, 0.3, 0.5)), (1, (1.0,))):
        base = run_fixed(device, enc, pairs, 1.0, scales, wts, g)
        got = run(device, enc, pairs, 1.0, ENGINE, scales, wts, g)
        assert same64(got[0], base[0]) and same64(got[1], base[1])
        for i in range(2):
            assert HM.same(got[2][i][0], base[2][i][0], enc) and HM.same(got[2][i][1], base[2][i][1], enc) and np.any(got[2][i][0] & 0x7FFF)
        # a NULL window through the _win entries themselves (the binding's window=None calls the entries without _win)
        arenas = []
        try:
            ins = upload_inputs(device, pairs)
            arenas.append(ins)
            out, up, gar = Arena(np.float64), Arena(np.float32), Arena(np.uint16)
            out.add((1, 1, 2))
            out.add((1, 1, 4 * scales))
            up.add((1, 1, 2), "dense", np.asarray(g, np.float32).reshape(1, 1, 2))
            idx = [[gar.add((d, h, w)) for _ in range(2)] for _ in range(2)]
            arenas += [out.upload(ctx), up.upload(ctx), gar.upload(ctx)]
            ps = (ssim_amd.Params3H * 2)()
            arrs = [(ssim_amd.Grad3H * 2)(), (ssim_amd.Grad3H * 2)()]
            for i in range(2):
                ps[i] = ssim_amd.make_params3h(w, h, d, ins.at(2 * i)[0], ins.at(2 * i)[1], ins.at(2 * i + 1)[0], ins.at(2 * i + 1)[1])
                for k in range(2):
                    arrs[k][i] = ssim_amd.Grad3H(gar.at(idx[k][i])[0], *gar.at(idx[k][i])[1])
            cw = None if wts is None else (ctypes.c_double * scales)(*wts)
            assert lib.rmgr_ssim_hip_enqueue_msssim3h_win(ctx.handle, 2, ps, code, 1.0, None, scales, cw, out.at(0)[0], out.at(1)[0]) == 0
            assert lib.rmgr_ssim_hip_enqueue_msssim3h_win_grad(ctx.handle, 2, ps, code, 1.0, None, scales, cw, out.at(1)[0], up.at(0)[0], arrs[0], arrs[1]) == 0
            call(ctx.synchronize)
            v, m = out.results(written=True)
            assert same64(v.reshape(2), base[0]) and same64(m.reshape(2, scales, 2), base[1])
            res = gar.results()
            for i in range(2):
                assert HM.same(res[idx[0][i]], base[2][i][0], enc) and HM.same(res[idx[1][i]], base[2][i][1], enc)
            fo, fm = (ctypes.c_float * 2)(), (ctypes.c_double * (4 * scales))()
            assert lib.rmgr_ssim_hip_compute_msssim3h_win_device(ctx.handle, 2, ps, code, 1.0, None, scales, cw, fo, fm) == 0
            assert np.array(fo[:], np.float32).tobytes() == base[0].astype(np.float32).tobytes()
            assert same64(np.array(fm[:], np.float64).reshape(2, scales, 2), base[1])
        finally:
            for a in arenas:
                a.free()


# ---- a strided view -----------------------------------------------------------------------------------------------------------------------

@ENC
@pytest.mark.parametrize("layout", ["negative sliceStride", "step 2", "odd offset", "stored (W, D, H)"])
def test_views_give_the_bits_of_the_dense_volume(device, enc, layout):
    assert layout in LAYOUTS
    size = (37, 19, 14)
    pair = IN.random_pair(size, 77, enc)
    g = [voxel_scale(size)]
    for window in (BOX3, G9):
        dense, _ = check_against_float32(device, enc, [pair], 1.0, window, 3, uniform(3), g, (window, "dense"))
        for lin, lout in ((layout, layout), (layout, "dense"), ("dense", layout)):
            v, m, gr = run(device, enc, [pair], 1.0, window, 3, uniform(3), g, lin=lin, lout=lout)
            assert same64(v, dense[0]) and same64(m, dense[1]), (window, lin, lout)
            assert HM.same(gr[0][0], dense[2][0][0], enc) and HM.same(gr[0][1], dense[2][0][1], enc), (window, lin, lout)


# ---- slices far apart ------------------------------------------------------------------------------------------------------------------

@ENC
@BY_RADIUS
def test_slices_two_to_the_22_elements_apart(device, enc, window):
    """One 9 x 5 x 3 pair at 2 scales whose slices lie 2^22 samples apart -- A, B and both gradients, each at its own place in one device
    buffer --, ascending and descending: the bits of the dense call, and nothing but the gradient volumes written."""
    ctx = device.ctx
    w, h, d, far = 9, 5, 3, 1 << 22
    pair = IN.random_pair((w, h, d), 33, enc)
    scales, wts, win = 2, (0.4, 0.6), mk(window)
    g = [45.0 * w * h * d]
    dense, _ = check_against_float32(device, enc, [pair], 1.0, window, scales, wts, g, "dense")
    room = 64                                                     # samples per item and slice (>= w * h)
    total = 2 * far + 4 * room
    sent = SENT[np.dtype(np.uint16)]

    def at(item, z):
        return z * far + item * room
    for sign in (1, -1):
        host = np.full(total, sent, np.uint16)
        z0 = 0 if sign == 1 else d - 1
        for item, vol in ((0, pair[0][::sign]), (1, pair[1][::sign])):
            for z in range(d):
                host[at(item, z):at(item, z) + w * h] = vol[z].reshape(-1)
        buf = ctx.upload(host)
        strides = (1, w, sign * far)
        ps = (ssim_amd.Params3H * 1)()
        ps[0] = ssim_amd.make_params3h(w, h, d, buf.ptr + 2 * at(0, z0), strides, buf.ptr + 2 * at(1, z0), strides)
        ga, gb = (ssim_amd.Grad3H * 1)(), (ssim_amd.Grad3H * 1)()
        ga[0], gb[0] = ssim_amd.Grad3H(buf.ptr + 2 * at(2, z0), *strides), ssim_amd.Grad3H(buf.ptr + 2 * at(3, z0), *strides)
        vals, means, go = ctx.alloc(8), ctx.alloc(16 * scales), ctx.upload(np.float32(g))
        call(ctx.enqueue_msssim3h, ps, 1, 1.0, enc, vals.ptr, means.ptr, scales, wts, win)
        call(ctx.enqueue_msssim3h_grad, ps, 1, 1.0, enc, means.ptr, go.ptr, ga, gb, scales, wts, win)
        call(ctx.synchronize)
        assert same64(vals.download(np.float64, (1,)), dense[0]) and same64(means.download(np.float64, (1, scales, 2)), dense[1])
        got = buf.download(np.uint16, (total,))
        for item, want in ((2, dense[2][0][0]), (3, dense[2][0][1])):
            vol = np.stack([got[at(item, z):at(item, z) + w * h].reshape(h, w) for z in range(d)])[::sign]
            assert HM.same(np.ascontiguousarray(vol), want, enc) and np.any(want & 0x7FFF), (item, sign)
            for z in range(d):
                got[at(item, z):at(item, z) + w * h] = host[at(item, z):at(item, z) + w * h]
        assert np.array_equal(got, host), "a sample outside the gradient volumes was written"
        for x in (buf, vals, means, go):
            x.free()


# ---- the single rounding ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [BOX3, G9], ids=MK.name_of)
def test_float16_subnormals_and_overflow_under_a_loss_scale(device, window):
    """gOut and 1024 gOut under a window: the result is round(1024 g), not 1024 round(g) -- the two differ exactly where round(g) is a
    float16 subnormal, and gOut puts the unscaled gradient there --; and a gOut that takes the largest voxels past 65504 gives +-Inf
    exactly where the rounded float32 gradient does."""
    enc = HM.F16
    size = (33, 20, 13)
    pair = IN.random_pair(size, 10, enc)
    got1, ref1 = check_against_float32(device, enc, [pair], 1.0, window, 3, uniform(3), [0.375], "unscaled")
    got2, ref2 = check_against_float32(device, enc, [pair], 1.0, window, 3, uniform(3), [1024.0 * 0.375], "scaled")
    assert np.any(HM.is_subnormal(got1[2][0][0], enc))
    scaled_after = HM.round_to(HM.widen(got1[2][0][0], enc) * np.float32(1024.0), enc)
    differ = got2[2][0][0] != scaled_after
    print("%s: %d of %d voxels differ between round(1024 g) and 1024 round(g)" % (MK.name_of(window), int(differ.sum()), differ.size))
    assert differ.any()
    top = float(np.abs(ref2[3][0][0]).max()) / (1024.0 * 0.375)
    got, ref = check_against_float32(device, enc, [pair], 1.0, window, 3, uniform(3), [4.0 * MAX16[enc] / top], "overflow")
    inf = (got[2][0][0] & 0x7FFF) == 0x7C00
    assert np.array_equal(inf, np.abs(ref[3][0][0]) >= 65520.0) and 0 < inf.sum() < inf.size
    assert np.all(np.isfinite(ref[3][0][0]))


# ---- the sample type ----------------------------------------------------------------------------------------------------------------------

def test_sample_type_zero_is_float16_and_anything_else_is_einval(device):
    ctx, lib = device.ctx, device.ctx.lib
    size = (17, 9, 5)
    w, h, d = size
    pair = IN.random_pair(size, 3, HM.F16)
    want = run(device, HM.F16, [pair], 1.0, BOX3, 2, uniform(2))
    ins = upload_inputs(device, [pair])
    try:
        ps = (ssim_amd.Params3H * 1)()
        ps[0] = ssim_amd.make_params3h(w, h, d, ins.at(0)[0], ins.at(0)[1], ins.at(1)[0], ins.at(1)[1])
        win = mk(BOX3)
        cw = (ctypes.c_double * 2)(0.5, 0.5)
        fo, fm = (ctypes.c_float * 1)(), (ctypes.c_double * 4)()
        assert ssim_amd.SAMPLE_F16 == 0
        assert lib.rmgr_ssim_hip_compute_msssim3h_win_device(ctx.handle, 1, ps, 0, 1.0, ctypes.byref(win), 2, cw, fo, fm) == 0
        assert np.float32(fo[0]).tobytes() == np.float32(want[0][0]).tobytes() and same64(np.array(fm[:], np.float64).reshape(1, 2, 2), want[1])
        for st in (2, 3, 0xFFFF, 0xFFFFFFFF):
            assert lib.rmgr_ssim_hip_compute_msssim3h_win_device(ctx.handle, 1, ps, st, 1.0, ctypes.byref(win), 2, cw, fo, fm) == errno.EINVAL
            assert lib.rmgr_ssim_hip_compute_msssim3h_win_device(ctx.handle, 1, ps, st, 1.0, None, 2, cw, fo, fm) == errno.EINVAL
    finally:
        ins.free()
