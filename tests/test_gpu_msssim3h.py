"""GPU: multi-scale SSIM of float16 / bfloat16 volumes and its gradient (rmgr_ssim_hip_*_msssim3h*, msssim3h_kernels.hip) against the
float32 entries, BIT FOR BIT.  Sizes are W x H x D; arrays are (D, H, W); 16-bit samples travel as uint16 bit patterns.

The contract (include/rmgr/ssim-hip.h): the value and both means of every scale have the bits rmgr_ssim_hip_enqueue_msssim3f gives on the
widened volumes; a gradient voxel is the float32 value _enqueue_msssim3f_grad would store at scale 0, rounded once, to nearest-even, into
the inputs' encoding.  So every comparison here runs the float32 entry in the same process on halfmodel.widen(samples) and compares bits
-- gradients against halfmodel.round_to(float32 gradient) -- and no tolerance is new.  NaN is compared as NaN.  The one comparison with a
bound is the golden volumes as stored against the float64 model at msssim3f_model.tolerances(); tests/test_msssim3h_cpu.py checks its
input condition (both encodings hold those volumes exactly, so the bounds' own inputs are these).

Every 16-bit call keeps its inputs, its gradient volumes, its values and its means in buffers with sentinel gaps (test_gpu_ssim3h.Arena);
after every call the gaps and every element of a strided buffer outside the volumes are asserted untouched.  After a return code that is
neither success nor EINVAL the module starts nothing more on the GPU (test_gpu_ssimk's _device_error, through test_gpu_ssim3h.call).

Cost, measured on an MI355X: the 95 tests other than test_sub_batches_of_the_forward (under 3 s per encoding) take 8.3 s together, the
PyTorch child process included; the device holds 1.5 GiB more than before the module at the peak (the backward sub-batch test's 1 GiB of
scratch and its 68 gradient pairs).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import content_classes as C
import halfmodel as HM
import msssim3f_model as M
import msssim3f_plan as MP
import ssim3f_chunks_inputs as CH
import ssim3f_model as S
import ssim3f_plan as P
import ssim3h_inputs as IN
import ssim_amd
from conftest import ROOT
from test_gpu_msssim3f import DROPPED, uniform
from test_gpu_msssim3f import run as run_f32
from test_gpu_ssim3h import LAYOUTS, MAX16, NAN16, Arena, Device, call
from test_gpu_ssimk import _device_error

pytestmark = pytest.mark.gpu

ENC = pytest.mark.parametrize("enc", HM.ENCODINGS)
SIZES = [(1, 1, 1), (3, 1, 2), (2, 5, 3), (17, 17, 9), (33, 20, 13), (37, 21, 44)]          # W x H x D
WEIGHT_SETS = [(5, None)] + [(n, uniform(n)) for n in range(1, M.MAX_SCALES + 1)] + [(3, (0.0, 0.5, 0.5))]


@pytest.fixture(scope="module")
def device(gpu_ctx):
    d = Device(gpu_ctx)
    yield d
    d.close()


def same64(x, y):
    """float64 arrays with the same bit patterns, NaN compared as NaN."""
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    xn, yn = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and np.array_equal(xn, yn) and np.array_equal(x[~xn].view(np.uint64), y[~yn].view(np.uint64))


def upload_inputs(device, pairs, lin="dense"):
    """An Arena holding a and b of every pair under the layout `lin`: volume 2 i is A of pair i, 2 i + 1 its B."""
    ins = Arena(np.uint16)
    for a, b in pairs:
        ins.add(a.shape, lin, a)
        ins.add(b.shape, lin, b)
    return ins.upload(device.ctx)


def run(device, enc, pairs, r, scales=5, weights=None, g_out=None, want=(True, True), lin="dense", lout="dense", inputs=None, ctx=None):
    """Forward (values, means) and -- g_out given -- backward of `pairs` (uint16 bit patterns) in ONE enqueue each, device-resident.
    inputs: (Arena from upload_inputs, [index of the pair each volume of the call names]) instead of pairs.  Returns (values float64 (n,),
    means float64 (n, scales, 2), [(dA or None, dB or None)] as uint16)."""
    ctx = device.ctx if ctx is None else ctx
    arenas = []
    try:
        if inputs is None:
            ins, names = upload_inputs(device, pairs, lin), list(range(len(pairs)))
            arenas.append(ins)
        else:
            ins, names = inputs
        n = len(names)
        d, h, w = ins.items[0][3].shape
        out = Arena(np.float64)
        out.add((1, 1, n))
        out.add((1, 1, 2 * n * scales))
        arenas.append(out.upload(ctx))
        ps = (ssim_amd.Params3H * n)()
        for i, k in enumerate(names):
            (pa, sa), (pb, sb) = ins.at(2 * k), ins.at(2 * k + 1)
            if lin == "odd offset" and i == 0:
                assert pa % 4 == 2, "the layout does not put the base address at 2 mod 4"
            ps[i] = ssim_amd.make_params3h(w, h, d, pa, sa, pb, sb)
        call(ctx.enqueue_msssim3h, ps, n, r, enc, out.at(0)[0], out.at(1)[0], scales, weights)
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
            call(ctx.enqueue_msssim3h_grad, ps, n, r, enc, out.at(1)[0], up.at(0)[0], arrs[0], arrs[1], scales, weights)
        call(ctx.synchronize)
        device.sample()
        v, m = out.results(written=True)
        grads = []
        if g_out is not None:
            got = gar.results()
            grads = [(got[idx[0][i]] if want[0] else None, got[idx[1][i]] if want[1] else None) for i in range(n)]
            up.results()
        if inputs is None:
            ins.results()                                  # the inputs and everything around them are unchanged
        return v.reshape(n), m.reshape(n, scales, 2), grads
    finally:
        for a in arenas:
            a.free()


def widened(pairs, enc):
    return [(HM.widen(a, enc), HM.widen(b, enc)) for a, b in pairs]


def reference(device, enc, pairs, r, scales, weights, g_out=None):
    """msssim3f on the widened volumes: (values, means, [(dA, dB) rounded once into the encoding])."""
    v, m, gr = run_f32(device.ctx, widened(pairs, enc), r, scales, weights, g_out)
    return v, m, [(HM.round_to(ga, enc), HM.round_to(gb, enc)) for ga, gb in gr], gr


def check_against_float32(device, enc, pairs, r, scales, weights, g_out, what, one_gradient=False, **kw):
    """One call of the 16-bit entries against the same call of the float32 entries on the widened volumes."""
    got = run(device, enc, pairs, r, scales, weights, g_out, **kw)
    ref = reference(device, enc, pairs, r, scales, weights, g_out)
    assert same64(got[0], ref[0]) and same64(got[1], ref[1]), (what, got[0], ref[0])
    assert len(got[2]) == len(ref[2]) == (len(pairs) if g_out is not None else 0)
    for (ga, gb), (fa, fb) in zip(got[2], ref[2]):
        assert ga.dtype == np.uint16 and HM.same(ga, fa, enc) and HM.same(gb, fb, enc), what
    if one_gradient:
        only_a = run(device, enc, pairs, r, scales, weights, g_out, want=(True, False), **kw)
        only_b = run(device, enc, pairs, r, scales, weights, g_out, want=(False, True), **kw)
        for i in range(len(pairs)):
            assert only_a[2][i][1] is None and only_b[2][i][0] is None
            assert HM.same(only_a[2][i][0], ref[2][i][0], enc) and HM.same(only_b[2][i][1], ref[2][i][1], enc), what
        assert same64(only_a[0], ref[0]) and same64(only_b[1], ref[1])
    return got, ref


def voxel_scale(size):
    """A dLoss/dMS of the order of the voxel count: the gradient of a mean is of order 1 / (W H D), which float16 would flush."""
    return -0.75 * float(size[0] * size[1] * size[2])


# ---- every size under every weight set ------------------------------------------------------------------------------------------------

@ENC
@pytest.mark.parametrize("size", SIZES, ids=CH.shape_id)
def test_value_means_and_gradients_have_the_float32_bits(device, enc, size):
    """(9, 17, 17) as (D, H, W) is two tiles in x and y and two reduction cells in z; every size is odd on some axis at some scale.  Wang's
    five, uniform weights at 1 .. 8 scales (one scale: the ssim form and kMsLast at scale 0) and (0, 0.5, 0.5), whose k_0 is 0: scale 0
    stores the rounded upstream share of scale 1.  Value, all means, dA alone, dB alone and both."""
    pair = IN.random_pair(size, 100 + sum(size), enc)
    for scales, weights in WEIGHT_SETS:
        got, ref = check_against_float32(device, enc, [pair], 1.0, scales, weights, [voxel_scale(size)], (size, scales, weights), one_gradient=True)
        if size != (1, 1, 1):
            assert np.abs(ref[3][0][0]).max() > 0 and np.any(got[2][0][0] & 0x7FFF), (size, scales)
        if weights is not None and weights[0] == 0.0:
            # the float32 gradient of scale 0 IS the upstream share: 0.125 c g_1(x >> 1, y >> 1, z >> 1); on a voxel away from the odd
            # borders the float32 gradient is constant over each 2 x 2 x 2 block
            f = ref[3][0][0]
            if min(f.shape) >= 2:
                assert f[0, 0, 0] == f[1, 1, 1] == f[0, 1, 0] and f[0, 0, 0] != 0


# ---- determinism ------------------------------------------------------------------------------------------------------------------------

@ENC
@pytest.mark.parametrize("size,scales", [((17, 17, 131), 3), ((5, 3, 1000), 4)], ids=lambda s: str(s))
def test_chunk_depths_of_every_scale_change_no_bit(device, enc, size, scales):
    """Launches of 1, 7 and 40 volumes: plan3f picks other chunk depths (asserted through tests/ssim3f_plan.py, per scale).  The volumes
    are drawn from seven distinct pairs and five dLoss/dMS values (ssim3f_chunks_inputs.picks); every value, mean and gradient has the
    bits of ITS OWN (pair, dLoss/dMS) combination launched alone, and one lone launch is held to the float32 path."""
    cus = device.cus
    counts = (1, 7, 40)
    depths = {k: [P.plan3f(*(MP.dims(*size, s) + (k, cus))).chunk_slices for s in range(scales)] for k in counts}
    print("chunk depths per scale on %d CUs: %r" % (cus, depths))
    assert depths[1][0] != depths[40][0] and len(set(depths[40])) > 1, depths
    pairs = [(HM.round_to(a, enc), HM.round_to(b, enc)) for a, b in CH.pairs(size)]
    g_outs = [g * float(size[0] * size[1] * size[2]) for g in CH.G_OUTS]
    ins = upload_inputs(device, pairs)
    try:
        lone = {}
        for n in counts[1:]:
            which, g_of = CH.picks(n, 3)
            combos = list(zip(which.tolist(), g_of.tolist()))
            assert all(x != y for x, y in zip(combos, combos[1:])), combos
            for c in sorted(set(combos)):
                if c not in lone:
                    lone[c] = run(device, enc, None, 1.0, scales, uniform(scales), [g_outs[c[1]]], inputs=(ins, [c[0]]))
            v, m, gr = run(device, enc, None, 1.0, scales, uniform(scales), [g_outs[c[1]] for c in combos], inputs=(ins, [c[0] for c in combos]))
            for i, c in enumerate(combos):
                assert same64(v[i:i + 1], lone[c][0]) and same64(m[i], lone[c][1][0]), (n, i, c)
                assert HM.same(gr[i][0], lone[c][2][0][0], enc) and HM.same(gr[i][1], lone[c][2][0][1], enc), (n, i, c)
        assert len(set(k for k, _ in lone)) == CH.PAIRS and len(lone) >= 30
        k, g = sorted(lone)[0]
        ref = reference(device, enc, [pairs[k]], 1.0, scales, uniform(scales), [g_outs[g]])
        assert same64(lone[(k, g)][0], ref[0]) and same64(lone[(k, g)][1], ref[1])
        assert HM.same(lone[(k, g)][2][0][0], ref[2][0][0], enc) and HM.same(lone[(k, g)][2][0][1], ref[2][0][1], enc)
        assert np.any(ref[2][0][0] & 0x7FFF)
    finally:
        ins.results()
        ins.free()


@ENC
def test_seven_pairs_in_one_call_and_the_same_call_twice(device, enc):
    size = (33, 20, 13)
    pairs = [IN.random_pair(size, 40 + i, enc) for i in range(7)]
    g = [x * float(33 * 20 * 13) for x in (-0.75, 1.5, 0.25, 1.0, -2.0, 0.5, 3.0)]
    alone = [run(device, enc, [pairs[i]], 1.0, 4, uniform(4), [g[i]]) for i in range(7)]
    ref = reference(device, enc, pairs, 1.0, 4, uniform(4), g)
    for attempt in range(2):
        v, m, gr = run(device, enc, pairs, 1.0, 4, uniform(4), g)
        assert same64(v, ref[0]) and same64(m, ref[1])
        for i in range(7):
            assert same64(v[i:i + 1], alone[i][0]) and same64(m[i], alone[i][1][0]), (i, attempt)
            assert HM.same(gr[i][0], alone[i][2][0][0], enc) and HM.same(gr[i][1], alone[i][2][0][1], enc), (i, attempt)
            assert HM.same(gr[i][0], ref[2][i][0], enc) and HM.same(gr[i][1], ref[2][i][1], enc), (i, attempt)


@ENC
def test_device_host_and_enqueue_entries_agree(device, enc):
    size = (37, 19, 14)
    ua, ub = IN.random_pair(size, 78, enc)
    v, m, _ = run(device, enc, [(ua, ub)], 1.0)
    rv, rm, _, _ = reference(device, enc, [(ua, ub)], 1.0, 5, None)
    assert same64(v, rv) and same64(m, rm)
    want = np.float32(v[0])
    (ha, st), (hb, _) = HM.host_array(ua, enc), HM.host_array(ub, enc)
    for ctx in (None, device.ctx):
        hv, hm = call(ssim_amd.compute_msssim3h, ha, hb, 1.0, st, 5, None, True, ctx)
        assert np.float32(hv).tobytes() == want.tobytes() and same64(hm, m[0])
    # the host entry stages views as they are: a transposed, reversed view of other storage
    ta, tb = np.ascontiguousarray(ha.transpose(1, 2, 0)[::-1]), np.ascontiguousarray(hb[:, :, ::-1])
    hv = call(ssim_amd.compute_msssim3h, ta[::-1].transpose(2, 0, 1), tb[:, :, ::-1], 1.0, st)
    assert np.float32(hv).tobytes() == want.tobytes()
    vs, ms = call(ssim_amd.compute_msssim3h_batch, [(ha, hb), (hb, ha), (ha, ha)], 1.0, st, 5, None, True, device.ctx)
    assert vs[:1].tobytes() == want.tobytes() and same64(ms[0], m[0]) and abs(float(vs[2]) - 1.0) < 1e-6
    ins = upload_inputs(device, [(ua, ub)])
    try:
        ps = (ssim_amd.Params3H * 1)()
        ps[0] = ssim_amd.make_params3h(size[0], size[1], size[2], ins.at(0)[0], ins.at(0)[1], ins.at(1)[0], ins.at(1)[1])
        dv, dm = call(device.ctx.msssim3h_device, ps, 1, 1.0, enc, 5, None, True)
        assert dv.tobytes() == np.float32([want]).tobytes() and same64(dm, m)
    finally:
        ins.free()


@ENC
@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "dense"])
def test_views_give_the_bits_of_the_dense_volume(device, enc, layout):
    """Negative step, stride and sliceStride, interleaved samples, permuted axes, and a base address that is 2 mod 4 (`odd offset`), which
    the float32 path cannot have: inputs and gradient volumes.  The Arena asserts every byte around the gradient samples untouched."""
    size = (37, 19, 14)
    pair = IN.random_pair(size, 77, enc)
    g = [voxel_scale(size)]
    dense = run(device, enc, [pair], 1.0, 3, uniform(3), g)
    ref = reference(device, enc, [pair], 1.0, 3, uniform(3), g)
    assert same64(dense[0], ref[0]) and HM.same(dense[2][0][0], ref[2][0][0], enc) and np.any(dense[2][0][0] & 0x7FFF)
    for lin, lout in ((layout, layout), (layout, "dense"), ("dense", layout)):
        v, m, gr = run(device, enc, [pair], 1.0, 3, uniform(3), g, lin=lin, lout=lout)
        assert same64(v, dense[0]) and same64(m, dense[1]), (lin, lout)
        assert HM.same(gr[0][0], dense[2][0][0], enc) and HM.same(gr[0][1], dense[2][0][1], enc), (lin, lout)
    # one scale as well: the kMsLast adjoint and the ssim-form walk through the same views
    one = run(device, enc, [pair], 1.0, 1, (1.0,), g)
    v, m, gr = run(device, enc, [pair], 1.0, 1, (1.0,), g, lin=layout, lout=layout)
    assert same64(v, one[0]) and HM.same(gr[0][0], one[2][0][0], enc) and HM.same(gr[0][1], one[2][0][1], enc)


# ---- sub-batches and shared scratch ---------------------------------------------------------------------------------------------------------

@ENC
def test_sub_batches_of_the_backward_scratch(device, enc):
    """test_gpu_msssim3f's test of the same name on 16-bit volumes: the scratch is float32 whatever the samples are, so one more volume of
    96^3 at two scales than a sub-batch of the backward for both gradients holds (tests/msssim3f_plan.py) makes two sub-batches.  Drawn
    from three pairs and three dLoss/dMS values; the volumes around the boundary differ from their neighbours in both.  Every value, mean
    and gradient has the bits of its own combination launched alone, and every lone launch those of the float32 path."""
    size, scales = (96, 96, 96), 2
    n = MP.per_sub_batch(*size, scales, 2) + 1
    assert n == 68 and MP.sub_batches(*size, scales, 2, n) == [(0, 67), (67, 1)]
    pairs = [IN.random_pair(size, 3 + k, enc) for k in range(3)]
    g_outs = [g * float(96 ** 3) for g in CH.G_OUTS[:3]]
    which, g_of = CH.picks(n, 5)
    combos = [(k % len(pairs), g % len(g_outs)) for k, g in zip(which.tolist(), g_of.tolist())]
    for i in (65, 66):                                           # the last two volumes of the first sub-batch, the only one of the second
        assert combos[i][0] != combos[i + 1][0] and combos[i][1] != combos[i + 1][1], combos[65:]
    assert len(set(combos)) == len(pairs) * len(g_outs)
    ins = upload_inputs(device, pairs)
    try:
        lone = {c: run(device, enc, None, 1.0, scales, uniform(scales), [g_outs[c[1]]], inputs=(ins, [c[0]])) for c in sorted(set(combos))}
        for k in range(len(pairs)):
            ref = reference(device, enc, [pairs[k]], 1.0, scales, uniform(scales), [g_outs[0]])
            assert same64(lone[(k, 0)][0], ref[0]) and same64(lone[(k, 0)][1], ref[1])
            assert HM.same(lone[(k, 0)][2][0][0], ref[2][0][0], enc) and HM.same(lone[(k, 0)][2][0][1], ref[2][0][1], enc)
        for c in lone:                                           # distinct pairs and distinct dLoss/dMS give distinct results
            assert np.any(lone[c][2][0][0] & 0x7FFF) and np.any(lone[c][2][0][1] & 0x7FFF)
            for o in lone:
                assert c == o or not np.array_equal(lone[c][2][0][0], lone[o][2][0][0]), (c, o)
        v, m, gr = run(device, enc, None, 1.0, scales, uniform(scales), [g_outs[c[1]] for c in combos], inputs=(ins, [c[0] for c in combos]))
        for i, c in enumerate(combos):
            assert same64(v[i:i + 1], lone[c][0]) and same64(m[i], lone[c][1][0]), (i, c)
            assert HM.same(gr[i][0], lone[c][2][0][0], enc) and HM.same(gr[i][1], lone[c][2][0][1], enc), (i, c)
    finally:
        ins.results()
        ins.free()


@ENC
def test_sub_batches_of_the_forward(device, enc):
    """test_gpu_msssim3f's test of the same name on 16-bit volumes: 65536 volumes of 2 x 1 x 3 at two scales, one more than a launch takes,
    drawn from five pairs; the only volume of the second sub-batch differs from its neighbour and from the first volume of the call.  Every
    value and mean has the bits of its pair launched alone, and every lone launch those of the float32 path."""
    size, scales = (2, 1, 3), 2
    n = MP.per_sub_batch(*size, scales, 0) + 1
    assert n == 65536 and MP.sub_batches(*size, scales, 0, n) == [(0, 65535), (65535, 1)]
    pairs = [IN.random_pair(size, 90 + k, enc) for k in range(5)]
    which = np.random.default_rng([CH.SEED, n]).permutation(np.arange(n) % len(pairs)).tolist()
    assert which[n - 1] != which[n - 2] and which[n - 1] != which[0]
    ins = upload_inputs(device, pairs)
    try:
        lone = [run(device, enc, None, 1.0, scales, uniform(scales), inputs=(ins, [k])) for k in range(len(pairs))]
        for k in range(len(pairs)):
            ref = reference(device, enc, [pairs[k]], 1.0, scales, uniform(scales))
            assert same64(lone[k][0], ref[0]) and same64(lone[k][1], ref[1])
            for o in range(k):                                   # distinct pairs give distinct values and means
                assert not same64(lone[k][0], lone[o][0]) and not same64(lone[k][1][0, 0], lone[o][1][0, 0]), (k, o)
        v, m, _ = run(device, enc, None, 1.0, scales, uniform(scales), inputs=(ins, which))
        pick = np.asarray(which)
        bad = np.flatnonzero((v.view(np.uint64) != np.concatenate([x[0] for x in lone])[pick].view(np.uint64)) |
                             np.any(m.view(np.uint64) != np.concatenate([x[1] for x in lone])[pick].view(np.uint64), axis=(1, 2)))
        assert len(bad) == 0, "%d of %d volumes differ from their pair launched alone; the first: volume %d" % (len(bad), n, bad[0])
    finally:
        ins.results()
        ins.free()


@ENC
def test_a_dozen_enqueues_share_the_scratch_in_stream_order(device, enc):
    """msssim3h forward and backward of two shapes mixed with msssim3f_grad, ssim3h_grad and the 2-D msssimh on one context without a host
    wait: every output byte equals the same call issued alone on a second context."""
    shapes = [(40, 36, 20), (21, 50, 33)]
    vols = [IN.random_pair(s, 60 + i, enc) for i, s in enumerate(shapes)]
    rng = np.random.default_rng(22)
    pa, pb = HM.round_to(rng.random((256, 272), dtype=np.float32), enc), HM.round_to(rng.random((256, 272), dtype=np.float32), enc)

    def issue(ctx, wait):
        assert not _device_error, "an earlier call left a device error: %r" % _device_error
        keep, outs, steps = [], {}, []
        for i, (a, b) in enumerate(vols):
            d, h, w = a.shape
            go = ctx.upload(np.float32([-0.75 * a.size]))
            va, vb = ctx.upload(a), ctx.upload(b)
            fa, fb = ctx.upload(HM.widen(a, enc)), ctx.upload(HM.widen(b, enc))
            keep += [go, va, vb, fa, fb]
            dense = (1, w, w * h)
            p3 = (ssim_amd.Params3H * 1)()
            p3[0] = ssim_amd.make_params3h(w, h, d, va.ptr, dense, vb.ptr, dense)
            f3 = (ssim_amd.Params3F * 1)()
            f3[0] = ssim_amd.make_params3f(w, h, d, fa.ptr, dense, fb.ptr, dense)
            sizes = {"v": 8, "m": 80, "ga": 2 * a.size, "gb": 2 * a.size, "sa": 2 * a.size, "fv": 8, "fm": 80, "fa": 4 * a.size}
            for k, nbytes in sizes.items():
                outs["%s%d" % (k, i)] = ctx.upload(np.full(nbytes, 0xA5, np.uint8))
            ga, gb, gs, gf = (ssim_amd.Grad3H * 1)(), (ssim_amd.Grad3H * 1)(), (ssim_amd.Grad3H * 1)(), (ssim_amd.Grad3F * 1)()
            ga[0], gb[0] = ssim_amd.Grad3H(outs["ga%d" % i].ptr, *dense), ssim_amd.Grad3H(outs["gb%d" % i].ptr, *dense)
            gs[0], gf[0] = ssim_amd.Grad3H(outs["sa%d" % i].ptr, *dense), ssim_amd.Grad3F(outs["fa%d" % i].ptr, *dense)
            keep += [p3, f3, ga, gb, gs, gf]
            # the float32 forward comes first, on its own, so that msssim3f_grad has means to read
            call(ctx.enqueue_msssim3f, f3, 1, 1.0, outs["fv%d" % i].ptr, outs["fm%d" % i].ptr)
            call(ctx.synchronize)
            steps.append([lambda p3=p3, i=i: ctx.enqueue_msssim3h(p3, 1, 1.0, enc, outs["v%d" % i].ptr, outs["m%d" % i].ptr),
                          lambda p3=p3, gs=gs, go=go: ctx.enqueue_ssim3h_grad(p3, 1, 1.0, enc, go.ptr, gs, None),
                          lambda p3=p3, i=i, ga=ga, gb=gb, go=go: ctx.enqueue_msssim3h_grad(p3, 1, 1.0, enc, outs["m%d" % i].ptr, go.ptr, ga, gb),
                          lambda f3=f3, i=i, gf=gf, go=go: ctx.enqueue_msssim3f_grad(f3, 1, 1.0, outs["fm%d" % i].ptr, go.ptr, gf, None)])
        da, db = ctx.upload(pa), ctx.upload(pb)
        keep += [da, db]
        p2 = (ssim_amd.Params16 * 1)()
        p2[0] = ssim_amd.make_params16(272, 256, da.ptr, 1, 272, db.ptr, 1, 272)
        outs["ms"], outs["means"] = ctx.upload(np.full(8, 0xA5, np.uint8)), ctx.upload(np.full(80, 0xA5, np.uint8))
        two_d = lambda: ctx.enqueue_msssimh(p2, 1, 1.0, enc, outs["ms"].ptr, outs["means"].ptr)      # noqa: E731
        s0, s1 = steps
        order = [s0[0], s1[0], two_d, s0[1], s1[2], s0[3], s0[2], two_d, s1[1], s1[3], s0[0], s1[2], s0[2], two_d]
        assert len(order) >= 12
        for step in order:
            call(step)
            if wait:
                call(ctx.synchronize)
        call(ctx.synchronize)
        got = {k: v.download(np.uint8, (v.nbytes,)) for k, v in outs.items()}
        for v in list(outs.values()) + [x for x in keep if hasattr(x, "free")]:
            v.free()
        return got
    mixed = issue(device.ctx, False)
    with ssim_amd.Context(0) as other:
        alone = issue(other, True)
    for k in alone:
        assert np.array_equal(alone[k], mixed[k]), k
        assert not np.all(mixed[k] == 0xA5), k
    assert np.any(mixed["ga0"].view(np.uint16) & 0x7FFF)


# ---- content ----------------------------------------------------------------------------------------------------------------------------------

def content_classes():
    """tests/content_classes.py on (12, 19, 40) without the classes tests/test_gpu_msssim3f.py leaves out (its DROPPED, and HUGE_CLASSES)."""
    return [c for c in C.volume_classes((12, 19, 40), 1.0) if c[0] not in C.HUGE_CLASSES and c[0] not in DROPPED]


@ENC
@pytest.mark.parametrize("name", [c[0] for c in content_classes()])
def test_content_classes_at_four_scales(device, enc, name):
    """Each class encoded, then compared with the float32 path on the widened volumes: whatever the encoding did to the class, both paths
    see the same samples.  The non-finite classes compare NaN as NaN."""
    _, a, b, r, _ = C.named(content_classes(), name)
    pair = (HM.round_to(a, enc), HM.round_to(b, enc))
    got, _ = check_against_float32(device, enc, [pair], r, 4, uniform(4), [-0.75 * a.size * r], name)
    if name == "anticorrelated":                                 # the ReLU case: value 0, every gradient voxel +0
        assert got[1][0][0][0] < 0 and got[0][0] == 0.0
        for g in got[2][0]:
            assert not np.any(g), "a gradient voxel is not +0"


@ENC
def test_nan_inf_subnormal_samples_and_a_zero_upstream_gradient(device, enc):
    size = (33, 20, 13)
    ua, ub = IN.random_pair(size, 5, enc)
    g = [voxel_scale(size)]
    for bad in (NAN16[enc], HM.round_to(np.float32([np.inf]), enc)[0]):
        x = ua.copy()
        x[6, 10, 16] = bad
        got, _ = check_against_float32(device, enc, [(x, ub)], 1.0, 3, uniform(3), g, "one bad sample")
        assert np.isnan(got[0][0]) and np.any(HM.is_nan(got[2][0][0], enc))
    # gOut = 0: every gradient voxel +0, even with a NaN sample
    x = ua.copy()
    x[2, 3, 4] = NAN16[enc]
    for vol in (ua, x):
        _, _, gr = run(device, enc, [(vol, ub)], 1.0, 3, uniform(3), [0.0])
        for t in gr[0]:
            assert not np.any(t), "a gradient voxel is not +0"
    if enc == HM.F16:
        # a volume of float16 subnormals (below 6.1e-5) at a data range of their order: kept, not flushed
        rng = np.random.default_rng(8)
        sa = rng.integers(1, 0x400, size=(13, 20, 33)).astype(np.uint16)
        sb = np.clip(sa.astype(np.int32) + rng.integers(-40, 41, size=sa.shape), 1, 0x3FF).astype(np.uint16)
        assert np.all(HM.is_subnormal(sa, enc)) and np.all(HM.is_subnormal(sb, enc))
        got, ref = check_against_float32(device, enc, [(sa, sb)], 6.0e-5, 3, uniform(3), [1e-4], "subnormal samples")
        assert 0.0 < got[0][0] < 1.0 and np.any(got[2][0][0] & 0x7FFF)
        flushed = run_f32(device.ctx, [(np.zeros(sa.shape, np.float32), np.zeros(sa.shape, np.float32))], 6.0e-5, 3, uniform(3))
        assert not same64(got[0], flushed[0])


def test_float16_overflows_to_inf_exactly_where_the_rounded_float32_gradient_does(device):
    enc = HM.F16
    size = (33, 20, 13)
    pair = IN.random_pair(size, 9, enc)
    _, _, _, f32 = reference(device, enc, [pair], 1.0, 3, uniform(3), [1.0])
    top = float(np.abs(f32[0][0]).max())
    g = [4.0 * MAX16[enc] / top]                                 # the largest quarter or so of the voxels pass 65504
    got, ref = check_against_float32(device, enc, [pair], 1.0, 3, uniform(3), g, "overflow")
    inf = (got[2][0][0] & 0x7FFF) == 0x7C00
    assert np.array_equal(inf, np.abs(ref[3][0][0]) >= 65520.0) and 0 < inf.sum() < inf.size
    assert np.all(np.isfinite(ref[3][0][0]))


@ENC
def test_a_loss_scale_arrives_before_the_single_rounding(device, enc):
    """gOut and 1024 gOut: the result is round(1024 g), not 1024 round(g).  A power of two commutes with the rounding of a normal number,
    so the two orders differ exactly where round(g) is subnormal in the encoding: gOut is chosen to put the unscaled gradient there
    (float16: below 6.1e-5; bfloat16: below 1.2e-38, where float32 still has some 19 bits against bfloat16's 3 or 4), and the test
    asserts that at least one voxel differs.  Both values of gOut are powers of two times 0.375: exact in float32."""
    size = (33, 20, 13)
    pair = IN.random_pair(size, 10, enc)
    base = 0.375 * (2.0 ** -115 if enc == HM.BF16 else 1.0)
    got1, ref1 = check_against_float32(device, enc, [pair], 1.0, 3, uniform(3), [base], "unscaled")
    got2, ref2 = check_against_float32(device, enc, [pair], 1.0, 3, uniform(3), [1024.0 * base], "scaled")
    scaled_after = HM.round_to(HM.widen(got1[2][0][0], enc) * np.float32(1024.0), enc)
    differ = got2[2][0][0] != scaled_after
    print("%s: %d of %d voxels differ between round(1024 g) and 1024 round(g)" % (enc, int(differ.sum()), differ.size))
    assert differ.any()
    assert HM.same(got2[2][0][0], HM.round_to(ref2[3][0][0], enc), enc)


# ---- the float64 model ----------------------------------------------------------------------------------------------------------------------

_golden = {}


def golden_model(manifest, name):
    """(float32 a, float32 b, value, means) of the float64 model on one stored golden volume; computed once for both encodings."""
    if name not in _golden:
        (_, a, b, r), = S.fixture_forms(manifest, name, ("raw",))
        assert r == 255.0
        _golden[name] = (a, b) + M.Model(a, b, r).msssim(5, None)
    return _golden[name]


@ENC
@pytest.mark.parametrize("name", S.FIXTURES)
def test_stored_golden_volumes_against_the_float64_model(device, manifest, enc, name):
    """The five golden volumes as stored (integers 0 .. 255, exact in both encodings: tests/test_msssim3h_cpu.py), range 255, Wang's five
    scales: value and means at msssim3f_model's bounds.  The forward is also held to the float32 path bit for bit; the gradient is held
    through the bit identity alone -- the float64 model does not round to 16 bits."""
    value_tol, mean_tol, _, _ = M.tolerances()
    a, b, gv, gm = golden_model(manifest, name)
    pair = (HM.round_to(a, enc), HM.round_to(b, enc))
    assert np.array_equal(HM.widen(pair[0], enc), a)
    (v, m, _), _ = check_against_float32(device, enc, [pair], 255.0, 5, None, [255.0 * a.size], name)
    dv, dm = abs(v[0] - gv), float(np.abs(m[0] - gm).max())
    print("%s %s: value %.3g (bound %.3g), means %.3g (bound %.3g)" % (name, enc, dv, value_tol, dm, mean_tol))
    assert dv <= value_tol and dm <= mean_tol, (name, dv, dm)


# ---- PyTorch ----------------------------------------------------------------------------------------------------------------------------------
# torch brings its own HIP runtime; the checks run in ONE child process (tests/tools/msssim3h_torch_checks.py) that imports torch before the
# library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    assert not _device_error, "an earlier call left a device error: %r" % _device_error
    tool = os.path.join(ROOT, "tests", "tools", "msssim3h_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "msssim3h_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["forward_and_backward_are_the_float32_path_rounded_once", "non_contiguous_and_expanded_inputs_are_read_in_place",
                                   "loss_under_autocast_reaches_a_bfloat16_leaf_as_bfloat16", "side_stream", "loss_forms_on_sixteen_bit_tensors",
                                   "refusals"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
