"""GPU: the gradient of the 3-D SSIM map for a per-voxel upstream gradient (rmgr_ssim_hip_enqueue_ssim3f_map_grad, ssim3w_kernels.hip) against
the float64 model of tests/ssim3w_model.py and against the entries of ssim3f it extends, and the bit patterns the header promises.  Sizes
are W x H x D; arrays are (D, H, W).

Bound.  Measured, not estimated: ssim3w_model.EMU_GRAD holds what an fp32 emulation of the two walks leaves against the float64 model on
the golden volumes under three weight volumes (tests/test_ssim3w_cpu.py pins it); everything here asserts twice that figure of the
volume's largest float64 gradient magnitude.  Nothing is compared against itself: bits against rmgr_ssim_hip_enqueue_ssim3f_grad or
against the dense, lone call; values against the float64 model.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ssim3f_model as S
import ssim3f_plan as P
import ssim3w_model as MW
import ssim_amd
from conftest import ROOT
from test_gpu_ssim3f import LAYOUTS, SENT, Vol, random_pair, same

pytestmark = pytest.mark.gpu

GRAD_TOL = MW.tolerances()


def random_k(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def params_of(inputs):
    d, h, w = inputs[0][0].shape
    ps = (ssim_amd.Params3F * len(inputs))()
    for i, (va, vb) in enumerate(inputs):
        ps[i] = ssim_amd.make_params3f(w, h, d, va.ptr, va.strides, vb.ptr, vb.strides)
    return ps


def backward(ctx, pairs, r, g_out=None, ks=None, want=(True, True), lin="dense", lk="dense", lout="dense", inputs=None, kvols=None, scalar_k=False):
    """ONE enqueue of the backward of `pairs`, device-resident: g_out given, rmgr_ssim_hip_enqueue_ssim3f_grad; else
    rmgr_ssim_hip_enqueue_ssim3f_map_grad with the weight volumes ks under layout lk (scalar_k: ks are floats, each one float in device
    memory under strides 0, 0, 0).  Returns [(dA or None, dB or None)].  inputs / kvols: Vols uploaded by the caller, instead."""
    own = inputs is None
    if own:
        inputs = [(Vol(ctx, a.shape, lin, a), Vol(ctx, b.shape, lin, b)) for a, b in pairs]
    n = len(inputs)
    shape = inputs[0][0].shape
    ps = params_of(inputs)
    gvols, arrs = [[], []], [None, None]
    for k in range(2):
        if want[k]:
            arrs[k] = (ssim_amd.Grad3F * n)()
            for i in range(n):
                gv = Vol(ctx, shape, lout)
                gvols[k].append(gv)
                arrs[k][i] = ssim_amd.Grad3F(gv.ptr, *gv.strides)
    held = []
    if g_out is not None:
        go = ctx.upload(np.asarray(g_out, np.float32).reshape(n))
        held.append(go)
        ctx.enqueue_ssim3f_grad(ps, n, r, go.ptr, arrs[0], arrs[1])
    else:
        ms = (ssim_amd.GradOut3F * n)()
        if scalar_k:
            one = ctx.upload(np.asarray(ks, np.float32).reshape(n))
            held.append(one)
            for i in range(n):
                ms[i] = ssim_amd.GradOut3F(one.ptr + 4 * i, 0, 0, 0)
        else:
            own_k = kvols is None
            if own_k:
                kvols = [Vol(ctx, shape, lk, k) for k in ks]
                held.extend(kvols)
            for i in range(n):
                ms[i] = ssim_amd.GradOut3F(kvols[i].ptr, *kvols[i].strides)
        ctx.enqueue_ssim3f_map_grad(ps, n, r, ms, arrs[0], arrs[1])
    ctx.synchronize()
    grads = [(gvols[0][i].result() if want[0] else None, gvols[1][i].result() if want[1] else None) for i in range(n)]
    for v in gvols[0] + gvols[1] + held:
        v.free()
    if own:
        for va, vb in inputs:
            va.free()
            vb.free()
    return grads


def same_grads(x, y):
    return all((p is None and q is None) or same(p, q) for p, q in zip(x, y))


WANTS = {1: (True, False), 2: (False, True), 3: (True, True)}


# ---- identity ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1, 1), (2, 1, 3), (16, 16, 8), (17, 17, 9), (33, 20, 13)], ids=lambda s: "%dx%dx%d" % s)
def test_constant_volume_has_the_bits_of_the_scalar_entry(gpu_ctx, size):
    """A volume of the constant float(gOut / voxels), and the one float under strides 0, 0, 0, against rmgr_ssim_hip_enqueue_ssim3f_grad
    for gOut: which = 1, 2, 3."""
    a, b = random_pair(size, 100 + sum(size))
    for g_out in (-0.75, 2.5):
        kc = MW.constant_volume(g_out, a.shape)
        for which, want in WANTS.items():
            ref = backward(gpu_ctx, [(a, b)], 1.0, g_out=[g_out], want=want)
            assert any(g is not None and np.abs(g).max() > 0 for g in ref[0])
            got = backward(gpu_ctx, [(a, b)], 1.0, ks=[kc], want=want)
            assert same_grads(got[0], ref[0]), (size, g_out, which, "constant volume")
            got = backward(gpu_ctx, [(a, b)], 1.0, ks=[kc.flat[0]], want=want, scalar_k=True)
            assert same_grads(got[0], ref[0]), (size, g_out, which, "one float, strides 0")


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.FIXTURES)
def test_model_on_the_golden_volumes(gpu_ctx, manifest, name):
    """Both forms under the three weight volumes of ssim3w_model (the seeds of its measure()): every voxel of both gradients within
    ssim3w_model.tolerances() of the float64 model, relative to the volume's largest float64 gradient magnitude."""
    seed = S.FIXTURES.index(name)
    for form, a, b, r in S.fixture_forms(manifest, name):
        va, vb = Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)
        for wname, k in MW.weight_volumes(a.shape, seed):
            got = backward(gpu_ctx, None, r, ks=[k], inputs=[(va, vb)])[0]
            errs = [float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(got, MW.grad_map(a, b, r, k))]
            print("%s %s %s: gradients %.3g %.3g of max|grad|" % (name, form, wname, errs[0], errs[1]))
            assert all(np.all(np.isfinite(g)) for g in got) and max(errs) <= GRAD_TOL, (name, form, wname, errs)
        va.free()
        vb.free()


# ---- chunk depth -------------------------------------------------------------------------------------------------------------------------

def test_same_bits_at_every_chunk_depth(gpu_ctx):
    """5 x 3 x 200 with random weights: alone against inside batches of 40 and of 300 volumes, which the planner walks at another chunk
    depth (asserted with tests/ssim3f_plan.py for this device's CU count before anything is compared)."""
    w, h, d = size = (5, 3, 200)
    said = re.search(r"(\d+) CUs", gpu_ctx.describe())
    assert said, gpu_ctx.describe()
    cus = int(said.group(1))
    depths = {n: P.plan3f(w, h, d, n, cus).chunk_slices for n in (1, 40, 300)}
    print("chunk_slices on %d CUs: %r" % (cus, depths))
    assert len(set(depths.values())) >= 2, depths
    pairs = [random_pair(size, 60 + i) for i in range(3)]
    ks = [random_k((d, h, w), 70 + i) for i in range(3)]
    inputs = [(Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b)) for a, b in pairs]
    kvols = [Vol(gpu_ctx, k.shape, "dense", k) for k in ks]
    alone = [backward(gpu_ctx, None, 1.0, inputs=[inputs[i]], kvols=[kvols[i]])[0] for i in range(3)]
    for i in range(3):
        want = MW.grad_map(pairs[i][0], pairs[i][1], 1.0, ks[i])
        assert max(float(np.abs(g - t).max() / np.abs(t).max()) for g, t in zip(alone[i], want)) <= GRAD_TOL
    for n in (40, 300):
        got = backward(gpu_ctx, None, 1.0, inputs=[inputs[(i + n) % 3] for i in range(n)], kvols=[kvols[(i + n) % 3] for i in range(n)])
        for i in range(n):
            assert same_grads(got[i], alone[(i + n) % 3]), (n, i)
    for v in [x for p in inputs for x in p] + kvols:
        v.free()


# ---- batch and sub-batch -----------------------------------------------------------------------------------------------------------------

def test_alone_or_anywhere_in_a_batch_on_a_second_call_with_one_gradient_or_both(gpu_ctx):
    size = (33, 20, 13)
    pairs = [random_pair(size, 40 + i) for i in range(3)]
    ks = [random_k(pairs[0][0].shape, 50 + i) for i in range(3)]
    alone = [backward(gpu_ctx, [pairs[i]], 1.0, ks=[ks[i]])[0] for i in range(3)]
    for i in range(3):
        want = MW.grad_map(pairs[i][0], pairs[i][1], 1.0, ks[i])
        assert max(float(np.abs(g - t).max() / np.abs(t).max()) for g, t in zip(alone[i], want)) <= GRAD_TOL
    for order in ((0, 1, 2), (2, 0, 1)):
        for call in range(2):                                  # a second call: the same bits
            for want in WANTS.values():
                got = backward(gpu_ctx, [pairs[i] for i in order], 1.0, ks=[ks[i] for i in order], want=want)
                for pos, i in enumerate(order):
                    for k in range(2):
                        assert (got[pos][k] is None) == (not want[k])
                        assert got[pos][k] is None or same(got[pos][k], alone[i][k]), (order, pos, call, want, k)


def test_sub_batches_of_the_coefficient_scratch(gpu_ctx):
    """16 bytes of coefficients per voxel for both gradients in sub-batches of 1 GiB: three volumes of 288^3 run as two and one
    (tests/ssim3f_plan.py restates take3f).  Every pair reads the same three device volumes; every gradient has the bits of the lone call."""
    w = h = d = 288
    n = 3
    assert P.sub_batches(w, h, d, n, P.grad_scratch(w, h, d, 3)) == [(0, 2), (2, 1)]
    a, b = random_pair((w, h, d), 3)
    k = random_k(a.shape, 4)
    va, vb, vk = Vol(gpu_ctx, a.shape, "dense", a), Vol(gpu_ctx, a.shape, "dense", b), Vol(gpu_ctx, a.shape, "dense", k)
    lone = backward(gpu_ctx, None, 1.0, inputs=[(va, vb)], kvols=[vk])[0]
    assert np.abs(lone[0]).max() > 0 and np.abs(lone[1]).max() > 0
    got = backward(gpu_ctx, None, 1.0, inputs=[(va, vb)] * n, kvols=[vk] * n)
    for i in range(n):
        assert same_grads(got[i], lone), i
    for v in (va, vb, vk):
        v.free()
    gpu_ctx.trim()


# ---- views of gMap -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "dense"])
def test_views_of_gmap_give_the_bits_of_the_dense_volume(gpu_ctx, layout):
    """Negative step, stride and sliceStride, interleaved weights (step 2) and a (D, H, W) view of weights stored (H, W, D), the gaps
    holding a sentinel: gMap alone under the layout, and gMap, the samples and the gradients all under it, against the dense call."""
    a, b = random_pair((37, 19, 14), 77)
    k = random_k(a.shape, 78)
    dense = backward(gpu_ctx, [(a, b)], 1.0, ks=[k])[0]
    want = MW.grad_map(a, b, 1.0, k)
    assert max(float(np.abs(g - t).max() / np.abs(t).max()) for g, t in zip(dense, want)) <= GRAD_TOL
    for lin, lk, lout in (("dense", layout, "dense"), (layout, layout, layout)):
        got = backward(gpu_ctx, [(a, b)], 1.0, ks=[k], lin=lin, lk=lk, lout=lout)[0]
        assert same_grads(got, dense), (lin, lk, lout)


def test_gmap_slices_more_than_32_bits_apart(gpu_ctx):
    """A 20 x 18 x 2 weight volume whose two slices lie 2^30 + 64 floats (4 GiB and 256 bytes) apart in one device-only buffer, in
    ascending and in descending order (sliceStride = -(2^30 + 64)): an offset truncated to 32 bits reads 64 floats into the other slice.
    The bits of the dense call."""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    w, h, d, far = 20, 18, 2, (1 << 30) + 64
    a, b = random_pair((w, h, d), 9)
    k = random_k(a.shape, 10)
    assert not np.array_equal(k[0], k[1])
    va, vb = Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b)
    dense = backward(ctx, None, 1.0, ks=[k], inputs=[(va, vb)])[0]
    buf = ctx.alloc(4 * (far + w * h))
    for sign in (1, -1):
        for z in range(d):
            plane = np.ascontiguousarray(k[::sign][z])               # slice z of the volume is stored at far * z (sign 1) or far * (d - 1 - z)
            assert lib.rmgr_ssim_hip_memcpy_h2d(ctx.handle, buf.ptr + 4 * z * far, plane.ctypes.data, plane.nbytes) == 0
        ga, gb = Vol(ctx, a.shape, "dense"), Vol(ctx, a.shape, "dense")
        ms, pa, pb = (ssim_amd.GradOut3F * 1)(), (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)()
        ms[0] = ssim_amd.GradOut3F(buf.ptr + (0 if sign == 1 else 4 * far), 1, w, sign * far)
        pa[0], pb[0] = ssim_amd.Grad3F(ga.ptr, *ga.strides), ssim_amd.Grad3F(gb.ptr, *gb.strides)
        ctx.enqueue_ssim3f_map_grad(params_of([(va, vb)]), 1, 1.0, ms, pa, pb)
        ctx.synchronize()
        assert same(ga.result(), dense[0]) and same(gb.result(), dense[1]), sign
        ga.free()
        gb.free()
    for v in (va, vb, buf):
        v.free()


# ---- reach -------------------------------------------------------------------------------------------------------------------------------

def box(shape, where, radius):
    m = np.zeros(shape, bool)
    m[tuple(slice(max(p - radius, 0), p + radius + 1) for p in where)] = True
    return m


@pytest.mark.parametrize("where", [(12, 13, 14), (0, 29, 0)], ids=lambda p: "z%d y%d x%d" % p)
def test_the_reach_of_a_nan_weight(gpu_ctx, where):
    """One NaN in gMap at an interior and at a corner voxel of 30 x 30 x 30: exactly the 11^3 gradient voxels around it, clipped to the
    volume, are NaN; every other voxel is finite and meets the model."""
    a, b = random_pair((30, 30, 30), 5)
    k = random_k(a.shape, 6)
    k[where] = np.nan
    got = backward(gpu_ctx, [(a, b)], 1.0, ks=[k])[0]
    want = MW.grad_map(a, b, 1.0, k)
    inside = box(a.shape, where, 5)
    for g, t in zip(got, want):
        assert np.array_equal(np.isnan(g), inside) and np.all(np.isfinite(g[~inside]))
        assert np.abs(g - t)[~inside].max() <= GRAD_TOL * np.abs(t[~inside]).max()


def test_a_zero_weight_does_not_hide_a_nan_sample(gpu_ctx):
    a, b = random_pair((30, 30, 30), 7)
    where = (14, 15, 16)
    a[where] = np.nan
    for k in (np.zeros(a.shape, np.float32), None):
        got = backward(gpu_ctx, [(a, b)], 1.0, ks=[0.0 if k is None else k], scalar_k=k is None)[0]
        for g in got:
            assert np.array_equal(np.isnan(g), box(a.shape, where, 10)) and np.all(g[~box(a.shape, where, 10)] == 0)


# ---- scratch in stream order -------------------------------------------------------------------------------------------------------------

def test_twenty_enqueues_share_the_scratch_and_the_descriptor_ring_in_stream_order(gpu_ctx):
    """On one context, 20 enqueues alternating rmgr_ssim_hip_enqueue_ssim3f_grad and _ssim3f_map_grad of two shapes with no host wait
    between them -- more than the 8 descriptor slots, every one rewriting the coefficient scratch: every output equals the same call
    issued alone, with a host wait, on another context."""
    ctx = gpu_ctx
    shapes = [(33, 20, 13), (20, 18, 40)]
    data = []
    for i, size in enumerate(shapes):
        a, b = random_pair(size, 200 + i)
        k = random_k(a.shape, 210 + i)
        data.append((Vol(ctx, a.shape, "dense", a), Vol(ctx, a.shape, "dense", b), Vol(ctx, a.shape, "dense", k), ctx.upload(np.float32([-0.75 + i])), a, b, k))

    def issue(c, calls, wait):
        # the output volumes first: an upload waits for its context's stream, and nothing may wait between the enqueues
        outs, keep = [(Vol(ctx, data[shape_i][0].shape, "dense"), Vol(ctx, data[shape_i][0].shape, "dense")) for shape_i, _ in calls], []
        for (shape_i, mapped), (ga, gb) in zip(calls, outs):
            va, vb, vk, go = data[shape_i][:4]
            ps, pa, pb = params_of([(va, vb)]), (ssim_amd.Grad3F * 1)(), (ssim_amd.Grad3F * 1)()
            pa[0], pb[0] = ssim_amd.Grad3F(ga.ptr, *ga.strides), ssim_amd.Grad3F(gb.ptr, *gb.strides)
            if mapped:
                ms = (ssim_amd.GradOut3F * 1)()
                ms[0] = ssim_amd.GradOut3F(vk.ptr, *vk.strides)
                c.enqueue_ssim3f_map_grad(ps, 1, 1.0, ms, pa, pb)
                keep.append(ms)
            else:
                c.enqueue_ssim3f_grad(ps, 1, 1.0, go.ptr, pa, pb)
            keep.extend((ps, pa, pb))
            if wait:
                c.synchronize()
        c.synchronize()
        got = [(ga.result(), gb.result()) for ga, gb in outs]
        for ga, gb in outs:
            ga.free()
            gb.free()
        return got
    kinds = [(0, False), (0, True), (1, False), (1, True)]
    ctx.synchronize()                                          # the uploads above, before another context's stream reads them
    with ssim_amd.Context(0) as other:
        alone = issue(other, kinds, True)
    for (shape_i, mapped), got in zip(kinds, alone):           # the lone calls are held to the float64 model
        a, b, k = data[shape_i][4:]
        want = MW.grad_map(a, b, 1.0, k) if mapped else S.grad(a, b, 1.0, -0.75 + shape_i)
        tol = GRAD_TOL if mapped else S.tolerances()[2]
        assert max(float(np.abs(g - t).max() / np.abs(t).max()) for g, t in zip(got, want)) <= tol, (shape_i, mapped)
    calls = [kinds[(i % 2) + 2 * ((i // 2) % 2)] for i in range(20)]
    assert len(calls) > 8 and all(calls[i][1] != calls[i + 1][1] for i in range(19))
    mixed = issue(ctx, calls, False)
    for i, call in enumerate(calls):
        assert same_grads(mixed[i], alone[kinds.index(call)]), (i, call)
    for item in data:
        for v in item[:4]:
            v.free()


# ---- PyTorch -----------------------------------------------------------------------------------------------------------------------------
# torch brings its own HIP runtime; the checks run in ONE child process (tests/tools/ssim3w_torch_checks.py) that imports torch before the
# library, and every test below reads its own verdict.

@pytest.fixture(scope="module")
def torch_checks():
    tool = os.path.join(ROOT, "tests", "tools", "ssim3w_torch_checks.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, "ssim3w_torch_checks exit %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("check", ["map_is_the_map_of_compute_ssim3f", "weighted_sum_against_the_model", "mean_over_the_volume_against_ssim3d",
                                   "non_contiguous_x_and_sliced_grad_out_are_read_in_place", "side_stream"])
def test_torch(torch_checks, check):
    assert torch_checks.get(check) == "ok", torch_checks.get(check, "the check did not run")
