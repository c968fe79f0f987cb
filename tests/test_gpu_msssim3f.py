"""GPU: multi-scale SSIM of float32 volumes and its gradient (rmgr_ssim_hip_*_msssim3f*, msssim3f_kernels.hip) against the float64 model of
tests/msssim3f_model.py, and the bit patterns the header promises.  Sizes are W x H x D; arrays are (D, H, W).

Bounds.  Measured, not estimated: msssim3f_model.EMU_* hold what an fp32 emulation of the kernels' arithmetic leaves against the float64
model on the golden volumes at Wang's five scales and at 1 .. 8 scales with uniform weights (tests/test_msssim3f_cpu.py pins them);
everything here asserts TOL_FACTOR = 2 times those figures -- the value, every per-scale mean, the gradient error over the volume's largest
float64 gradient magnitude, and max|grad| * W * H * D * R / |gOut| on identical volumes.  Every input used for accuracy has m_s >= 0.2 at
every scale with a weight (checked on the CPU, tests/test_msssim3f_cpu.py).
"""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import content_classes as C
import msssim3f_model as M
import msssim3f_plan as MP
import ssim3f_chunks_inputs as CH
import ssim3f_model as S
import ssim3f_plan as P
import ssim_amd
from conftest import ROOT
from test_gpu_ssim3f import LAYOUTS, Vol, random_pair, same
from test_gpu_ssim3f import run as run_single

pytestmark = pytest.mark.gpu

VALUE_TOL, MEAN_TOL, GRAD_TOL, IDENT_TOL = M.tolerances()
WORST = {"value": 0.0, "mean": 0.0, "grad": 0.0, "ident": 0.0}

# The content classes the accuracy test leaves out (tests/test_msssim3f_cpu.py: the emulation's own figure on the class is above 85 % of an
# EMU bound), each with that figure.  At most two.
DROPPED = {
    # every sample above the range: the centre is 0, nothing is centred.  Emulated: value 2.87, mean 8.43, gradient 3.61 times EMU
    "offset above the range": (2.87, 8.43, 3.61),
    # C1 and C2 of order 1e-16 under samples of order 1.  Emulated: value 0.24, mean 1.26, gradient 0.75 times EMU
    "unit data at range 1e-6": (0.24, 1.26, 0.75),
}


def uniform(n):
    return (1.0 / n,) * n


@pytest.fixture(scope="module", autouse=True)
def module_report(gpu_ctx):
    """Prints what the module measured: seconds, peak device memory in use, the largest figure seen against each EMU bound."""
    info0 = ssim_amd.memory_info(gpu_ctx)
    t0 = time.time()
    yield
    print("\nmsssim3f: %.1f s; memory_info before %r after %r; largest figures: value %.3g (EMU %.3g), mean %.3g (EMU %.3g), gradient %.3g "
          "(EMU %.3g), identical %.3g (EMU %.3g)" % (time.time() - t0, info0, ssim_amd.memory_info(gpu_ctx), WORST["value"], M.EMU_VALUE,
                                                     WORST["mean"], M.EMU_MEAN, WORST["grad"], M.EMU_GRAD, WORST["ident"], M.EMU_IDENT))


def run(ctx, pairs, r, scales=5, weights=None, g_out=None, want=(True, True), lin="dense", lout="dense", inputs=None):
    """Forward (values, means) and -- g_out given -- backward of `pairs` in ONE enqueue each, device-resident.  Returns (values float64 (n,),
    means float64 (n, scales, 2), [(dA or None, dB or None)]).  inputs: (Vol of A, Vol of B) per pair, uploaded by the caller."""
    n = len(pairs) if inputs is None else len(inputs)
    own = inputs is None
    if own:
        inputs = [(Vol(ctx, a.shape, lin, a), Vol(ctx, b.shape, lin, b)) for a, b in pairs]
    d, h, w = inputs[0][0].shape
    ps = (ssim_amd.Params3F * n)()
    for i, (va, vb) in enumerate(inputs):
        ps[i] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides)
    values, means = ctx.alloc(8 * n), ctx.alloc(16 * n * scales)
    ctx.enqueue_msssim3f(ps, n, r, values.ptr, means.ptr, scales, weights)
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
        ctx.enqueue_msssim3f_grad(ps, n, r, means.ptr, go.ptr, arrs[0], arrs[1], scales, weights)
    ctx.synchronize()
    v, m = values.download(np.float64, (n,)), means.download(np.float64, (n, scales, 2))
    grads = [(gvols[0][i].result() if want[0] else None, gvols[1][i].result() if want[1] else None) for i in range(n)] if g_out is not None else []
    for x in gvols[0] + gvols[1] + ([go] if g_out is not None else []) + [values, means]:
        x.free()
    if own:
        for va, vb in inputs:
            va.free()
            vb.free()
    return v, m, grads


def check_model(ctx, a, b, r, scales, weights, what, g_out=-0.75, model=None, one_gradient=True, exclude=None):
    """Value, every per-scale mean and both gradients against the float64 model at TOL_FACTOR times the emulation's figures; a gradient
    has the same bits alone and together with the other."""
    model = M.Model(a, b, r) if model is None else model
    gv, gm = model.msssim(scales, weights)
    ga, gb = model.grad(g_out, scales, weights)
    vox = S.voxels(a.shape)
    v, m, both = run(ctx, [(a, b)], r, scales, weights, [g_out])
    if one_gradient:
        _, _, only_a = run(ctx, [(a, b)], r, scales, weights, [g_out], want=(True, False))
        _, _, only_b = run(ctx, [(a, b)], r, scales, weights, [g_out], want=(False, True))
        assert same(both[0][0], only_a[0][0]) and same(both[0][1], only_b[0][1]), what
    dv, dm = abs(v[0] - gv), float(np.abs(m[0] - gm).max())
    identical = np.array_equal(a, b)
    errs = []
    for got, wnt in ((both[0][0], ga), (both[0][1], gb)):
        keep = np.ones(a.shape, bool) if exclude is None else ~exclude
        assert np.all(np.isfinite(got[keep])), what
        if identical:
            errs.append(float(np.abs(got).max()) * vox * r / abs(g_out))
        else:
            errs.append(float(np.abs(got - wnt)[keep].max() / np.abs(wnt)[keep].max()))
    print("%s: value %.3g, means %.3g, gradients %.3g %.3g%s" % (what, dv, dm, errs[0], errs[1], " (identical: max|grad| W H D R)" if identical else ""))
    WORST["value"], WORST["mean"] = max(WORST["value"], dv), max(WORST["mean"], dm)
    WORST["ident" if identical else "grad"] = max(WORST["ident" if identical else "grad"], max(errs))
    assert dv <= VALUE_TOL and dm <= MEAN_TOL, (what, dv, dm)
    assert max(errs) <= (IDENT_TOL if identical else GRAD_TOL), (what, errs)
    return v, m, both


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.FIXTURES)
def test_model_on_the_golden_volumes_at_wangs_scales(gpu_ctx, manifest, name):
    forms = S.fixture_forms(manifest, name)
    assert len(forms) == 2
    for form, a, b, r in forms:
        check_model(gpu_ctx, a, b, r, 5, None, "%s %s" % (name, form), g_out=1.0, one_gradient=form == "unit")


def test_model_at_one_to_eight_scales_and_a_zero_weight(gpu_ctx, manifest):
    _, a, b, r = S.fixture_forms(manifest, "bbb257x65_q50_ch1")[0]
    model = M.Model(a, b, r)
    for n in range(1, M.MAX_SCALES + 1):
        check_model(gpu_ctx, a, b, r, n, uniform(n), "%d scales, uniform" % n, model=model, one_gradient=False)
    # a zero weight in the middle: that scale's means are reported, its local gradient is +0
    w = (0.25, 0.25, 0.0, 0.25, 0.25)
    _, m, _ = check_model(gpu_ctx, a, b, r, 5, w, "a zero weight", model=model)
    assert abs(m[0][2][0] - model.means(5)[2][0]) <= MEAN_TOL


def test_identical_volumes(gpu_ctx, manifest):
    _, a, _, r = S.fixture_forms(manifest, "einstein_blur")[0]
    v, m, _ = check_model(gpu_ctx, a, a, r, 5, None, "einstein_blur against itself", g_out=1.0)
    assert abs(v[0] - 1.0) <= VALUE_TOL


@pytest.mark.parametrize("size,scales", [((33, 20, 13), 5), ((17, 17, 9), 5), ((16, 16, 8), 4), ((37, 21, 44), 8)], ids=lambda s: str(s))
def test_model_on_random_pairs(gpu_ctx, size, scales):
    """Odd at several scales; across a tile and a cell; exactly one tile and one cell; eight scales down to 1 x 1 x 1."""
    a, b = random_pair(size, sum(size))
    check_model(gpu_ctx, a, b, 1.0, scales, uniform(scales), "%dx%dx%d at %d scales" % (size + (scales,)))


def test_tiny_shapes(gpu_ctx):
    one = np.full((1, 1, 1), 0.375, np.float32)
    for n in range(1, M.MAX_SCALES + 1):
        v, m, g = run(gpu_ctx, [(one, one)], 1.0, n, uniform(n), [1.0])
        assert abs(v[0] - 1.0) <= VALUE_TOL and np.all(np.abs(m - 1.0) <= MEAN_TOL), (n, v, m)      # cs = A2 rcp(A2): 1 to an ulp of fp32
        assert np.all(np.isfinite(g[0][0])) and np.all(np.isfinite(g[0][1]))
    for size in ((2, 1, 3), (3, 2, 1), (1, 1, 1)):
        a, b = random_pair(size, 7 + sum(size))
        for n in (1, 2, 3):
            check_model(gpu_ctx, a, b, 1.0, n, uniform(n), "%dx%dx%d at %d scales" % (size + (n,)), one_gradient=False)


# ---- bit identities -------------------------------------------------------------------------------------------------------------------------

def test_mssim_of_every_scale_is_ssim3f_on_the_pyramid(gpu_ctx):
    a, b = random_pair((37, 21, 44), 11)
    _, m, _ = run(gpu_ctx, [(a, b)], 1.0, 8, uniform(8))
    pa, pb = M.pyramid(a, 8, np.float32), M.pyramid(b, 8, np.float32)
    for s in range(8):
        assert pa[s].dtype == np.float32
        sums, _, _ = run_single(gpu_ctx, [(pa[s], pb[s])], 1.0, maps=False)
        assert same(np.float64([sums[0] / S.voxels(pa[s].shape)]), m[0, s, 1:2]), s


def test_one_scale_is_the_map_gradient_under_a_constant(gpu_ctx):
    ctx = gpu_ctx
    a, b = random_pair((33, 20, 13), 12)
    d, h, w = a.shape
    g_out = np.float32(-0.75)
    v, m, grads = run(ctx, [(a, b)], 1.0, 1, (1.0,), [g_out])
    ms = float(m[0, 0, 1]) ** 1.0
    assert same(np.float64([ms]), v)
    k0 = np.float32((((float(g_out) * 1.0) * ms) / float(m[0, 0, 1])) / (float(w) * float(h) * float(d)))
    va, vb, ga, gb, kd = Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b), Vol(ctx, a.shape), Vol(ctx, a.shape), ctx.upload(np.float32([k0]))
    ps, gm, pa, pb = (ssim_amd.Params3F * 1)(), (ssim_amd.GradOut3F * 1)(), (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)()
    ps[0] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides)
    gm[0], pa[0], pb[0] = ssim_amd.GradOut3F(kd.ptr, 0, 0, 0), ssim_amd.Grad3F(ga.ptr, *ga.strides), ssim_amd.Grad3F(gb.ptr, *gb.strides)
    ctx.enqueue_ssim3f_map_grad(ps, 1, 1.0, gm, pa, pb)
    ctx.synchronize()
    assert same(ga.result(), grads[0][0]) and same(gb.result(), grads[0][1]) and np.abs(grads[0][0]).max() > 0
    for x in (va, vb, ga, gb, kd):
        x.free()


# ---- determinism ----------------------------------------------------------------------------------------------------------------------------

def test_seven_pairs_in_one_call_and_the_same_call_twice(gpu_ctx):
    size = (33, 20, 13)
    pairs = [random_pair(size, 40 + i) for i in range(7)]
    g = [-0.75, 1.5, 0.25, 1.0, -2.0, 0.5, 3.0]
    alone = [run(gpu_ctx, [pairs[i]], 1.0, 4, uniform(4), [g[i]]) for i in range(7)]
    for call in range(2):
        v, m, gr = run(gpu_ctx, pairs, 1.0, 4, uniform(4), g)
        for i in range(7):
            assert same(v[i:i + 1], alone[i][0]) and same(m[i], alone[i][1][0]), (i, call)
            assert same(gr[i][0], alone[i][2][0][0]) and same(gr[i][1], alone[i][2][0][1]), (i, call)


@pytest.mark.parametrize("size,scales", [((17, 17, 131), 3), ((5, 3, 1000), 4)], ids=lambda s: str(s))
def test_chunk_depths_of_every_scale_change_no_bit(gpu_ctx, size, scales):
    """Launches of 1 and of 40 volumes: plan3f picks other chunk depths (asserted through tests/ssim3f_plan.py, per scale).  The 40 are
    drawn from seven distinct pairs and five dLoss/dS values (ssim3f_chunks_inputs.picks: neighbours differ), so that a volume-index
    mix-up in the pyramid, the coarse gradient pyramids, k_s or the coefficient scratch of any scale shows: every value, mean and
    gradient has the bits of ITS OWN (pair, dLoss/dS) combination launched alone.  One lone value and gradient against the float64
    model."""
    n = 40
    cus = int(re.search(r"(\d+) CUs", gpu_ctx.describe()).group(1))
    depths = {k: [P.plan3f(*(MP.dims(*size, s) + (k, cus))).chunk_slices for s in range(scales)] for k in (1, n)}
    print("chunk depths per scale on %d CUs: %r" % (cus, depths))
    assert depths[1][0] != depths[n][0] and len(set(depths[n])) > 1, depths
    pairs = CH.pairs(size)
    which, g_of = CH.picks(n, 3)
    combos = list(zip(which.tolist(), g_of.tolist()))
    assert len(set(which.tolist())) == CH.PAIRS and len(set(combos)) >= 30 and all(x != y for x, y in zip(combos, combos[1:])), combos
    vols = [(Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)) for a, b in pairs]
    lone = {c: run(gpu_ctx, None, 1.0, scales, uniform(scales), [CH.G_OUTS[c[1]]], inputs=[vols[c[0]]]) for c in sorted(set(combos))}
    k, g = combos[0]
    model = M.Model(pairs[k][0], pairs[k][1], 1.0)
    value, means = model.msssim(scales, uniform(scales))
    assert min(float(means[s][1] if s == scales - 1 else means[s][0]) for s in range(scales)) >= 0.2, means      # the bounds' input condition
    assert abs(lone[(k, g)][0][0] - value) <= VALUE_TOL
    errs = [float(np.abs(got - want).max() / np.abs(want).max()) for got, want in zip(lone[(k, g)][2][0], model.grad(CH.G_OUTS[g], scales, uniform(scales)))]
    print("pair %d at dLoss/dS %g alone: value %.3g (bound %.3g), gradients %.3g %.3g (bound %.3g)" % (
        k, CH.G_OUTS[g], abs(lone[(k, g)][0][0] - value), VALUE_TOL, errs[0], errs[1], GRAD_TOL))
    assert max(errs) <= GRAD_TOL, errs
    v, m, gr = run(gpu_ctx, None, 1.0, scales, uniform(scales), [CH.G_OUTS[c[1]] for c in combos], inputs=[vols[c[0]] for c in combos])
    for i, c in enumerate(combos):
        assert same(v[i:i + 1], lone[c][0]) and same(m[i], lone[c][1][0]), (i, c)
        assert same(gr[i][0], lone[c][2][0][0]) and same(gr[i][1], lone[c][2][0][1]), (i, c)
    for va, vb in vols:
        va.free()
        vb.free()


@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "dense"])
def test_views_give_the_bits_of_the_dense_volume(gpu_ctx, layout):
    a, b = random_pair((37, 19, 14), 77)
    dense = run(gpu_ctx, [(a, b)], 1.0, 3, uniform(3), [-0.75])
    for lin, lout in ((layout, layout), (layout, "dense"), ("dense", layout)):
        v, m, gr = run(gpu_ctx, [(a, b)], 1.0, 3, uniform(3), [-0.75], lin=lin, lout=lout)
        assert same(v, dense[0]) and same(m, dense[1]), (lin, lout)
        assert same(gr[0][0], dense[2][0][0]) and same(gr[0][1], dense[2][0][1]), (lin, lout)


def test_device_host_and_enqueue_entries_agree(gpu_ctx):
    a, b = random_pair((37, 19, 14), 78)
    v, m, _ = run(gpu_ctx, [(a, b)], 1.0)
    want = np.float32(v[0])
    for ctx in (None, gpu_ctx):
        hv, hm = ssim_amd.compute_msssim3f(a, b, 1.0, per_scale=True, ctx=ctx)
        assert same(np.float32([hv]), np.float32([want])) and same(hm, m[0])
    ta, tb = np.ascontiguousarray(a.transpose(1, 2, 0)[::-1]), np.ascontiguousarray(b[:, :, ::-1])
    hv = ssim_amd.compute_msssim3f(ta[::-1].transpose(2, 0, 1), tb[:, :, ::-1], 1.0)
    assert same(np.float32([hv]), np.float32([want]))
    vs, ms = ssim_amd.compute_msssim3f_batch([(a, b), (b, a), (a, a)], 1.0, per_scale=True)
    assert same(vs[:1], np.float32([want])) and same(ms[0], m[0]) and abs(float(vs[2]) - 1.0) < 1e-6
    va, vb = Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)
    ps = (ssim_amd.Params3F * 1)()
    ps[0] = ssim_amd.make_params3f(37, 19, 14, va.ptr, va.strides, vb.ptr, vb.strides)
    dv, dm = gpu_ctx.msssim3f_device(ps, 1, 1.0, per_scale=True)
    assert same(dv, np.float32([want])) and same(dm, m)
    va.free()
    vb.free()


# ---- sub-batches and shared scratch ---------------------------------------------------------------------------------------------------------

def test_sub_batches_of_the_backward_scratch(gpu_ctx):
    """One more volume of 96^3 at two scales than a sub-batch of the backward for both gradients holds (tests/msssim3f_plan.py): two
    sub-batches.  The volumes are drawn (ssim3f_chunks_inputs.picks) from three distinct pairs, 21 MB of inputs, and three dLoss/dS
    values; the volumes around the sub-batch boundary differ from their neighbours in pair and in dLoss/dS, so that an offset into the
    means, the dLoss/dS vector, the descriptors or the scratch that forgets the sub-batch's first volume shows.  Every value, mean and
    gradient has the bits of its own (pair, dLoss/dS) combination launched alone."""
    size, scales = (96, 96, 96), 2
    n = MP.per_sub_batch(*size, scales, 2) + 1
    assert n == 68 and MP.sub_batches(*size, scales, 2, n) == [(0, 67), (67, 1)]
    pairs = [random_pair(size, 3 + k) for k in range(3)]
    g_outs = CH.G_OUTS[:3]
    which, g_of = CH.picks(n, 5)
    combos = [(k % len(pairs), g % len(g_outs)) for k, g in zip(which.tolist(), g_of.tolist())]
    for i in (65, 66):                                           # the last two volumes of the first sub-batch, the only one of the second
        assert combos[i][0] != combos[i + 1][0] and combos[i][1] != combos[i + 1][1], combos[65:]
    assert len(set(combos)) == len(pairs) * len(g_outs)
    vols = [(Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)) for a, b in pairs]
    lone = {c: run(gpu_ctx, None, 1.0, scales, uniform(scales), [g_outs[c[1]]], inputs=[vols[c[0]]]) for c in sorted(set(combos))}
    for c in lone:
        assert np.abs(lone[c][2][0][0]).max() > 0 and np.abs(lone[c][2][0][1]).max() > 0
    for c in lone:                                               # distinct pairs and distinct dLoss/dS give distinct results
        for o in lone:
            assert c == o or not same(lone[c][2][0][0], lone[o][2][0][0]), (c, o)
    v, m, gr = run(gpu_ctx, None, 1.0, scales, uniform(scales), [g_outs[c[1]] for c in combos], inputs=[vols[c[0]] for c in combos])
    for i, c in enumerate(combos):
        assert same(v[i:i + 1], lone[c][0]) and same(m[i], lone[c][1][0]), (i, c)
        assert same(gr[i][0], lone[c][2][0][0]) and same(gr[i][1], lone[c][2][0][1]), (i, c)
    for va, vb in vols:
        va.free()
        vb.free()


def test_sub_batches_of_the_forward(gpu_ctx):
    """One more volume of 2 x 1 x 3 at two scales than a sub-batch of the forward holds (tests/msssim3f_plan.py: at this size the launch
    limit ends it, long before the scratch does): sub-batches of 65535 volumes and of one, in one enqueue.  The volumes are drawn from five
    distinct pairs; the only volume of the second sub-batch differs from its neighbour and from the first volume of the call, so that an
    offset into the values, the means or the descriptors that forgets the sub-batch's first volume shows.  Every value and mean has the
    bits of its pair launched alone."""
    size, scales = (2, 1, 3), 2
    n = MP.per_sub_batch(*size, scales, 0) + 1
    assert n == 65536 and MP.sub_batches(*size, scales, 0, n) == [(0, 65535), (65535, 1)]
    pairs = [random_pair(size, 90 + k) for k in range(5)]
    which = np.random.default_rng([CH.SEED, n]).permutation(np.arange(n) % len(pairs)).tolist()
    assert which[n - 1] != which[n - 2] and which[n - 1] != which[0]
    vols = [(Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)) for a, b in pairs]
    lone = [run(gpu_ctx, None, 1.0, scales, uniform(scales), inputs=[vols[k]]) for k in range(len(pairs))]
    for k in range(len(pairs)):                                  # distinct pairs give distinct values and means
        for o in range(k):
            assert not same(lone[k][0], lone[o][0]) and not same(lone[k][1][0, 0], lone[o][1][0, 0]), (k, o)
    v, m, _ = run(gpu_ctx, None, 1.0, scales, uniform(scales), inputs=[vols[k] for k in which])
    pick = np.asarray(which)
    bad = np.flatnonzero((v.view(np.uint64) != np.concatenate([lone[k][0] for k in range(len(pairs))])[pick].view(np.uint64)) |
                         np.any(m.view(np.uint64) != np.concatenate([lone[k][1] for k in range(len(pairs))])[pick].view(np.uint64), axis=(1, 2)))
    assert len(bad) == 0, "%d of %d volumes differ from their pair launched alone; the first: volume %d" % (len(bad), n, bad[0])
    for va, vb in vols:
        va.free()
        vb.free()


def test_a_dozen_enqueues_share_the_scratch_in_stream_order(gpu_ctx):
    """msssim3f forward and backward of two shapes mixed with ssim3f_grad and msssimf on one context without a host wait: every output byte
    equals the same call issued alone on another context."""
    shapes = [(40, 36, 20), (21, 50, 33)]
    vols = [random_pair(s, 60 + i) for i, s in enumerate(shapes)]
    rng = np.random.default_rng(22)
    pa, pb = rng.random((256, 272), dtype=np.float32), rng.random((256, 272), dtype=np.float32)

    def issue(ctx, wait):
        keep, outs, steps = [], {}, []
        go = ctx.upload(np.float32([-0.75]))
        keep.append(go)
        for i, (a, b) in enumerate(vols):
            d, h, w = a.shape
            va, vb = Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b)
            keep += [va, vb]
            p3 = (ssim_amd.Params3F * 1)()
            p3[0] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides)
            for k in ("v", "m", "ga", "gb", "sa"):
                outs["%s%d" % (k, i)] = ctx.alloc({"v": 8, "m": 80}.get(k, 4 * a.size))
            ga, gb, gs = (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)()
            ga[0], gb[0] = ssim_amd.Grad3F(outs["ga%d" % i].ptr, 1, w, w * h), ssim_amd.Grad3F(outs["gb%d" % i].ptr, 1, w, w * h)
            gs[0] = ssim_amd.Grad3F(outs["sa%d" % i].ptr, 1, w, w * h)
            keep += [p3, ga, gb, gs]
            steps.append((i, [lambda p3=p3, i=i: ctx.enqueue_msssim3f(p3, 1, 1.0, outs["v%d" % i].ptr, outs["m%d" % i].ptr),
                              lambda p3=p3, gs=gs: ctx.enqueue_ssim3f_grad(p3, 1, 1.0, go.ptr, gs, None),
                              lambda p3=p3, i=i, ga=ga, gb=gb: ctx.enqueue_msssim3f_grad(p3, 1, 1.0, outs["m%d" % i].ptr, go.ptr, ga, gb)]))
        da, db = ctx.upload(pa), ctx.upload(pb)
        keep += [da, db]
        p2 = (ssim_amd.ParamsF * 1)()
        p2[0] = ssim_amd.make_params_f(272, 256, da.ptr, 1, 272, db.ptr, 1, 272)
        outs["ms"], outs["means"] = ctx.alloc(8), ctx.alloc(80)
        two_d = lambda: ctx.enqueue_msssimf(p2, 1, 1.0, outs["ms"].ptr, outs["means"].ptr)      # noqa: E731
        order = [steps[0][1][0], steps[1][1][0], two_d, steps[0][1][1], steps[1][1][2], steps[0][1][2], two_d, steps[1][1][1],
                 steps[0][1][0], steps[1][1][2], steps[0][1][2], two_d]
        assert len(order) == 12
        for step in order:
            step()
            if wait:
                ctx.synchronize()
        ctx.synchronize()
        got = {k: v.download(np.uint8, (v.nbytes,)) for k, v in outs.items()}
        for v in list(outs.values()) + [x for x in keep if hasattr(x, "free")]:
            v.free()
        return got
    mixed = issue(gpu_ctx, False)
    with ssim_amd.Context(0) as other:
        alone = issue(other, True)
    for k in alone:
        assert np.array_equal(alone[k], mixed[k]), k
    assert np.abs(mixed["ga0"].view(np.float32)).max() > 0


# ---- content ----------------------------------------------------------------------------------------------------------------------------------

def content_classes():
    return [c for c in C.volume_classes((12, 19, 40), 1.0) if c[0] not in C.HUGE_CLASSES]


@pytest.mark.parametrize("name", [c[0] for c in content_classes() if c[0] not in C.NONFINITE_CLASSES and c[0] != "anticorrelated" and c[0] not in DROPPED])
def test_content_classes_at_four_scales(gpu_ctx, name):
    _, a, b, r, _ = C.named(content_classes(), name)
    check_model(gpu_ctx, a, b, r, 4, uniform(4), name, one_gradient=False)


def test_anticorrelated_is_the_relu_case(gpu_ctx):
    _, a, b, r, _ = C.named(content_classes(), "anticorrelated")
    v, m, gr = run(gpu_ctx, [(a, b)], r, 4, uniform(4), [1.0])
    assert M.Model(a, b, r).means(4)[0][0] < 0 and m[0][0][0] < 0
    assert v[0] == 0.0
    for g in gr[0]:
        assert not np.any(g.view(np.uint32)), "a gradient voxel is not +0"


def test_nan_and_inf_samples_and_a_zero_upstream_gradient(gpu_ctx):
    a, b = random_pair((33, 20, 13), 5)
    for bad in (np.nan, np.inf):
        x = a.copy()
        x[6, 10, 16] = bad
        v, _, _ = run(gpu_ctx, [(x, b)], 1.0, 3, uniform(3))
        assert np.isnan(v[0]), bad
    # gOut = 0: every gradient voxel +0, even with a NaN sample
    x = a.copy()
    x[2, 3, 4] = np.nan
    for vol in (a, x):
        _, _, gr = run(gpu_ctx, [(vol, b)], 1.0, 3, uniform(3), [0.0])
        for g in gr[0]:
            assert not np.any(g.view(np.uint32)), "a gradient voxel is not +0"


# ---- PyTorch ----------------------------------------------------------------------------------------------------------------------------------
# torch brings its own HIP runtime; the checks run in ONE child process (tests/tools/msssim3f_torch_checks.py) that imports torch before the
# library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "msssim3f_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "msssim3f_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["value_and_gradients_against_the_c_abi", "loss_forms_and_errors", "non_contiguous_and_expanded_inputs", "side_stream",
                                   "empty_batch"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
