"""CPU: the gradient of the 3-D SSIM map for a per-voxel upstream gradient -- the definition and its boundaries (include/rmgr/ssim-hip.h,
rmgr_ssim_hip_enqueue_ssim3f_map_grad, ssim_amd.torch_ops.ssim3d_map).  Sizes are W x H x D; arrays are (D, H, W).

  * the float64 model (tests/ssim3w_model.py) agrees with an independent restatement -- torch float64, F.conv3d on replicate-padded input,
    autograd of sum(k * map) -- within 1e-9, down to 1 x 1 x 1, and with the constant volume gOut / (W H D) it is ssim3f_model.grad;
  * the fp32 emulation of the two walks gives ssim3f_model.emulate_fp32's gradients bit for bit on the constant volume of the identity
    clause, and leaves the figure ssim3w_model.EMU_GRAD holds, pinned from both sides;
  * a zero weight does not hide a NaN sample, and a NaN weight reaches the 11 x 11 x 11 voxels around it, in the model and the emulation;
  * the entry point is exported and declared, every EINVAL comes before the device, a valid call without a device is ENODEV, and
    ssim_amd.torch_ops.ssim3d_map refuses what it documents before any GPU call;
  * the new kernels never spill, keep four waves per SIMD and 17504 B of LDS, and there are three of them.
"""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import ssim3f_model as S
import ssim3w_model as MW
import ssim_amd
from conftest import ROOT

FN = "rmgr_ssim_hip_enqueue_ssim3f_map_grad"
SIZES = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (5, 3, 4), (13, 12, 11)]


def _torch_restatement(a, b, data_range, k):
    """(dA, dB) of sum(k * map) by torch float64: 1-D conv3d per axis on replicate-padded volumes, the five statistics, autograd."""
    import torch
    import torch.nn.functional as Fn
    g = torch.tensor(S.gaussian_taps(), dtype=torch.float64)
    c1, c2 = S.constants(data_range)

    def blur(v):
        v = v[None, None]
        v = Fn.conv3d(Fn.pad(v, (5, 5, 0, 0, 0, 0), mode="replicate"), g.reshape(1, 1, 1, 1, 11))
        v = Fn.conv3d(Fn.pad(v, (0, 0, 5, 5, 0, 0), mode="replicate"), g.reshape(1, 1, 1, 11, 1))
        v = Fn.conv3d(Fn.pad(v, (0, 0, 0, 0, 5, 5), mode="replicate"), g.reshape(1, 1, 11, 1, 1))
        return v[0, 0]
    ta = torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    tb = torch.tensor(np.asarray(b, np.float64), requires_grad=True)
    ma, mb = blur(ta), blur(tb)
    s_aa, s_bb, s_ab = blur(ta * ta) - ma * ma, blur(tb * tb) - mb * mb, blur(ta * tb) - ma * mb
    m = (2 * ma * mb + c1) * (2 * s_ab + c2) / ((ma * ma + mb * mb + c1) * (s_aa + s_bb + c2))
    (torch.tensor(np.asarray(k, np.float64)) * m).sum().backward()
    return ta.grad.numpy(), tb.grad.numpy()


def _pair(size, seed):
    w, h, d = size
    rng = np.random.default_rng(seed)
    a = rng.random((d, h, w)).astype(np.float32)
    b = np.clip(a + 0.1 * rng.standard_normal((d, h, w)), 0, 1).astype(np.float32)
    return a, b, rng


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_model_is_the_conv3d_restatement(size):
    a, b, rng = _pair(size, size[0] * 100 + size[1] * 10 + size[2])
    k = rng.standard_normal(a.shape)
    for r, sa, sb in ((1.0, a, b), (255.0, a * np.float32(255), b * np.float32(255))):
        da, db = MW.grad_map(sa, sb, r, k)
        tda, tdb = _torch_restatement(sa, sb, r, k)
        assert np.abs(da - tda).max() <= 1e-9 and np.abs(db - tdb).max() <= 1e-9, (size, r)
        assert np.abs(tda).max() > 1e-6 / r                      # a gradient worth comparing


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_constant_volume_is_the_gradient_of_the_mean(size):
    a, b, _ = _pair(size, 7)
    for g_out in (-0.75, 2.5):
        want = S.grad(a, b, 1.0, g_out)
        got = MW.grad_map(a, b, 1.0, np.full(a.shape, g_out / S.voxels(a.shape)))
        for g, wt in zip(got, want):
            assert np.abs(g - wt).max() <= 1e-15 * max(np.abs(wt).max(), 1e-300), (size, g_out)


def test_emulation_with_the_constant_volume_is_the_ssim3f_emulation_bit_for_bit(manifest):
    cases = [(fa, fb, r) for _, fa, fb, r in S.fixture_forms(manifest, "bbb255x63_q50_ch1")]
    for size in ((1, 1, 1), (5, 3, 4), (33, 20, 13)):
        a, b, _ = _pair(size, 11)
        cases.append((a, b, 1.0))
    for fa, fb, r in cases:
        for g_out in (-0.75, 1.0):
            _, _, ea, eb = S.emulate_fp32(fa, fb, r, g_out)
            wa, wb = MW.emulate_fp32_map_grad(fa, fb, r, MW.constant_volume(g_out, fa.shape))
            assert np.array_equal(wa.view(np.uint32), ea.view(np.uint32)) and np.array_equal(wb.view(np.uint32), eb.view(np.uint32)), (fa.shape, r, g_out)


def test_fp32_emulation_leaves_the_pinned_figure(manifest):
    """emulate_fp32_map_grad against grad_map on the golden volumes of ssim3f_model (FIXTURES x FORMS) under the three weight volumes of
    ssim3w_model.weight_volumes, every voxel, both gradients.  Measured: 3.04e-4 of the volume's largest float64 gradient magnitude (the
    standard-normal weights on bbb255x63_q50_ch1 raw).  tests/test_gpu_ssim3w.py asserts twice ssim3w_model.EMU_GRAD."""
    got = MW.measure(manifest)
    print("emulation: grad %.3g" % got)
    assert got <= MW.EMU_GRAD, (got, MW.EMU_GRAD)
    # pinned from below as well: a figure that moved far away means the emulation no longer restates these kernels
    assert got >= MW.EMU_GRAD / 2, (got, MW.EMU_GRAD)
    assert MW.tolerances() == 2.0 * MW.EMU_GRAD


def test_reach_of_a_nan_weight_and_of_a_nan_sample_under_zero_weights():
    """k sits inside Gt: a NaN weight at p reaches the 11 x 11 x 11 gradient voxels around p, clipped; k(p) d(p) is a plain product: a NaN
    sample under an all-zero gMap still gives NaN on the 21 x 21 x 21 voxels around it -- in the model and in the emulation."""
    a, b, rng = _pair((30, 28, 26), 5)

    def box(where, radius):
        m = np.zeros(a.shape, bool)
        m[tuple(slice(max(p - radius, 0), p + radius + 1) for p in where)] = True
        return m
    for where in ((12, 13, 14), (0, 27, 3)):
        k = rng.standard_normal(a.shape).astype(np.float32)
        k[where] = np.nan
        for g in MW.grad_map(a, b, 1.0, k) + MW.emulate_fp32_map_grad(a, b, 1.0, k):
            assert np.array_equal(np.isnan(g), box(where, 5)) and np.all(np.isfinite(g[~box(where, 5)])), where
        an = a.copy()
        an[where] = np.nan
        for g in MW.grad_map(an, b, 1.0, np.zeros(a.shape)) + MW.emulate_fp32_map_grad(an, b, 1.0, np.zeros(a.shape, np.float32)):
            assert np.array_equal(np.isnan(g), box(where, 10)) and np.all(g[~box(where, 10)] == 0), where


# ---- the C ABI's validation (no device needed) ----

def _params(a, b, n=1, **over):
    ps = (ssim_amd.Params3F * n)()
    d, h, w = a.shape
    for i in range(n):
        ps[i] = ssim_amd.make_params3f(w, h, d, a.ctypes.data, (1, w, w * h), b.ctypes.data, (1, w, w * h))
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _grads(a, n=1):
    gs = (ssim_amd.Grad3F * n)()
    for i in range(n):
        gs[i] = ssim_amd.Grad3F(a.ctypes.data, 1, a.shape[2], a.shape[2] * a.shape[1])
    return gs


def _maps(k, n=1, strides=None):
    ms = (ssim_amd.GradOut3F * n)()
    for i in range(n):
        ms[i] = ssim_amd.GradOut3F(k.ctypes.data, *((1, k.shape[2], k.shape[2] * k.shape[1]) if strides is None else strides))
    return ms


def test_entry_point_is_exported_and_declared(lib):
    assert hasattr(lib, FN) and FN in ssim_amd.C_SYMBOLS
    assert hasattr(ssim_amd, "GradOut3F") and hasattr(ssim_amd.Context, "enqueue_ssim3f_map_grad")
    assert ctypes.sizeof(ssim_amd.GradOut3F) == 4 * ctypes.sizeof(ctypes.c_void_p)
    from ssim_amd import torch_ops
    assert callable(torch_ops.ssim3d_map)
    assert lib.rmgr_ssim_hip_get_abi_version() == 6
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    assert FN in header and "rmgr_ssim_hip_GradOut3F" in header
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    # no longer a follow-up of the volume family: the header's sentence and the README's bullet
    follow = re.search(r"Follow-ups, not in this interface: a caller-chosen window \(the _win entries\), float16 / bfloat16 volumes(.*?)\*/", header, re.S)
    assert follow and "per-voxel" not in follow.group(1), follow
    follow = re.search(r"- Follow-ups, not in this change: the configurable window \(size, sigma, box\), 16-bit samples(.*?)\n\n", readme, re.S)
    assert follow and "upstream gradient" not in follow.group(1), follow


def test_every_einval_comes_before_the_device(lib):
    a = np.zeros((6, 20, 30), np.float32)
    b = np.zeros((6, 20, 30), np.float32)
    ga = np.zeros((6, 20, 30), np.float32)
    k = np.zeros((6, 20, 30), np.float32)
    fake_ctx = ctypes.c_void_p(1)                                              # never dereferenced
    E = errno.EINVAL
    f = getattr(lib, FN)

    def rc(count=1, params=None, r=1.0, maps=0, ctx=fake_ctx, grads=None):
        n = max(count, 1)
        ps = _params(a, b, n) if params is None else params
        ms = _maps(k, n) if maps == 0 else maps
        ga_, gb_ = (_grads(ga, n), None) if grads is None else grads
        return f(ctx, count, ps, r, ms, ga_, gb_)
    # every EINVAL of _enqueue_ssim3f_grad
    assert rc(count=0) == E
    assert f(fake_ctx, 1, None, 1.0, _maps(k), _grads(ga), None) == E           # params NULL
    for dim in ("width", "height", "depth"):
        assert rc(params=_params(a, b, **{dim: 0})) == E
        assert rc(params=_params(a, b, **{dim: 0x7FFF0001})) == E              # above the kernels' limit
        two = _params(a, b, 2)
        setattr(two[1], dim, getattr(two[1], dim) - 1)
        assert rc(count=2, params=two) == E                                    # sizes differ
    bad = _params(a, b)
    bad[0].imgA.topLeft = None
    assert rc(params=bad) == E
    bad = _params(a, b, 2)
    bad[1].imgB.topLeft = None
    assert rc(count=2, params=bad) == E
    for off in (1, 2, 3):
        bad = _params(a, b)
        bad[0].imgA.topLeft = a.ctypes.data + off                              # not 4-byte aligned
        assert rc(params=bad) == E
        bad = _params(a, b, 2)
        bad[1].imgB.topLeft = b.ctypes.data + off
        assert rc(count=2, params=bad) == E
    for r in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert rc(r=r) == E
    assert rc(ctx=None) == E and rc(ctx=None, r=255.0) == E                    # the entry needs a context
    assert rc(grads=(None, None)) == E                                         # both gradient arrays NULL
    g = _grads(ga, 2)
    g[1].topLeft = None
    assert rc(count=2, grads=(g, None)) == E and rc(count=2, grads=(None, g)) == E
    g = _grads(ga)
    g[0].topLeft = ga.ctypes.data + 2
    assert rc(grads=(g, None)) == E and rc(grads=(_grads(ga), g)) == E
    # its own: a NULL gradOutMaps, a gMap topLeft that is NULL or not 4-byte aligned
    assert rc(maps=None) == E
    m = _maps(k, 2)
    m[1].topLeft = None
    assert rc(count=2, maps=m) == E
    for off in (1, 2, 3):
        m = _maps(k)
        m[0].topLeft = k.ctypes.data + off
        assert rc(maps=m) == E
    assert rc(maps=_maps(k, strides=(0, 0, 0)), ctx=None) == E                 # valid but for the context: nothing was dereferenced


def test_valid_call_without_a_device_fails_loudly(lib):
    """The entry takes a context and nothing else (there is no _host form), and without a device no context exists: creating one is
    ENODEV, through the C ABI and through the binding.  With a device, one valid call: a single float with all strides 0 as gMap."""
    if ssim_amd.device_count() > 0:
        a = np.full((4, 8, 8), 0.25, np.float32)
        with ssim_amd.Context(0) as ctx:
            da, dk, dg = ctx.upload(a), ctx.upload(np.ones(1, np.float32)), ctx.upload(np.full((4, 8, 8), 7.0, np.float32))
            ps, gm, gs = (ssim_amd.Params3F * 1)(), (ssim_amd.GradOut3F * 1)(), (ssim_amd.Grad3F * 1)()
            ps[0] = ssim_amd.make_params3f(8, 8, 4, da.ptr, (1, 8, 64), da.ptr, (1, 8, 64))
            gm[0], gs[0] = ssim_amd.GradOut3F(dk.ptr, 0, 0, 0), ssim_amd.Grad3F(dg.ptr, 1, 8, 64)
            ctx.enqueue_ssim3f_map_grad(ps, 1, 1.0, gm, gs, None)
            ctx.synchronize()
            g = dg.download(np.float32, (4, 8, 8))
            for d in (da, dk, dg):
                d.free()
        assert np.abs(g).max() < 1e-5                                          # a flat pair against itself: SSIM is at its maximum
        return
    handle = ctypes.c_void_p()
    assert lib.rmgr_ssim_hip_create(ctypes.byref(handle), 0, None) == errno.ENODEV and not handle
    with pytest.raises(ssim_amd.SsimError) as e:
        ssim_amd.Context(0)
    assert e.value.errno == errno.ENODEV


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 1, 8, 16, 16)
    with pytest.raises(ValueError, match="ssim3d_map: .*GPU"):
        torch_ops.ssim3d_map(x, x)                                             # CPU tensors
    with pytest.raises(TypeError, match="ssim3d_map"):
        torch_ops.ssim3d_map(x.double(), x.double())
    for t in (x.half(), x.bfloat16()):
        with pytest.raises(TypeError, match="ssim3d_map: .*float32 for now"):
            torch_ops.ssim3d_map(t, t)
        with pytest.raises(TypeError, match="float32 for now"):
            torch_ops.ssim3d_map(x, t)
    with pytest.raises(TypeError):
        torch_ops.ssim3d_map(x.numpy(), x.numpy())
    with pytest.raises(ValueError, match="ssim3d_map"):
        torch_ops.ssim3d_map(x, torch.zeros(2, 1, 8, 16, 15))
    with pytest.raises(ValueError, match="D, H, W"):
        torch_ops.ssim3d_map(torch.zeros(16, 16), torch.zeros(16, 16))         # fewer than 3 dimensions
    with pytest.raises(ValueError):
        torch_ops.ssim3d_map(torch.zeros(2, 0, 4, 4), torch.zeros(2, 0, 4, 4))     # empty volumes
    for r in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            torch_ops.ssim3d_map(x, x, r)
    with pytest.raises(ValueError, match="^ssim3d: "):
        torch_ops.ssim3d(x, x)                                                 # ssim3d still speaks in its own name


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; assert 'torch' not in sys.modules; "
                        "assert callable(ssim_amd.torch_ops.ssim3d_map)" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_map_gradient_walks_never_spill_and_keep_their_occupancy():
    """Build-time guard, as tests/test_ssim3f_cpu.py has for ssim3f_kernels.hip: exactly three kernels (dA, dB, both), nothing spills,
    each keeps four waves per SIMD (at most 128 VGPRs) and at most 17504 B of LDS -- the budget of the ssim3f coefficient walks they copy."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "ssim3w_kernels.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src), "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key in ("VGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]", "LDS Size \\[bytes/block\\]"):
            m = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if m and name:
                kernels[name][key.split(" ")[0]] = int(m.group(1))
    assert len(kernels) == 3 and all("ssim3w_walk" in k for k in kernels), sorted(kernels)
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0 and v["VGPRs"] <= 128 and v["Occupancy"] >= 4 and v["LDS"] <= 17504, (k, v)
