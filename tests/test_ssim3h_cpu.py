"""CPU: SSIM of float16 / bfloat16 volumes, its gradient and the gradient of its map -- the boundaries of the interface
(include/rmgr/ssim-hip.h, rmgr_ssim_hip_*_ssim3h*; ssim_amd.torch_ops.ssim3d_amp / ssim3d_map_amp).  Sizes are W x H x D; arrays are
(D, H, W).

  * the five entry points are exported, declared and listed; the structs have the size of four pointers; the ABI version stays 6;
  * every EINVAL comes back with a context that is never dereferenced: what ssim3f / ssim3f_map_grad refuse, odd byte addresses for
    samples and gradients (2-byte alignment is enough for them), 2-byte-but-not-4-byte addresses for the map and gMap, a sampleType that
    is neither constant;
  * _host without a device is ENODEV;
  * make_params3h and compute_ssim3h take the strides of negative, permuted and step-2 views in samples;
  * torch_ops refuses what it documents before any GPU call, ssim3d / ssim3d_map still say "float32 for now", the import stays torch-free;
  * the kernels: exactly 20, none spills, the walks and the adjoint walks keep the budgets of ssim3f's (plan3f assumes them);
  * the input condition of the GPU module's comparison with the float64 model: on the golden-derived volumes as stored in each
    encoding, the fp32 emulation of the kernels stays within half of ssim3f_model.tolerances() of the float64 model.
"""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import halfmodel as HM
import ssim3f_model as S
import ssim3h_inputs as IN
import ssim_amd
from conftest import ROOT

FNS = ("rmgr_ssim_hip_enqueue_ssim3h", "rmgr_ssim_hip_compute_ssim3h_device", "rmgr_ssim_hip_compute_ssim3h_host",
       "rmgr_ssim_hip_enqueue_ssim3h_grad", "rmgr_ssim_hip_enqueue_ssim3h_map_grad")
F16, BF16 = ssim_amd.SAMPLE_F16, ssim_amd.SAMPLE_BF16


def test_entry_points_are_exported_declared_and_listed(lib):
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    for fn in FNS:
        assert hasattr(lib, fn) and fn in ssim_amd.C_SYMBOLS and fn + "(" in header, fn
    for name in ("rmgr_ssim_hip_Img3H", "rmgr_ssim_hip_Params3H", "rmgr_ssim_hip_Grad3H"):
        assert "} %s;" % name in header, name
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(ssim_amd.Img3H) == 4 * ptr and ctypes.sizeof(ssim_amd.Grad3H) == 4 * ptr
    assert ctypes.sizeof(ssim_amd.Params3H) == ctypes.sizeof(ssim_amd.Params3F)
    assert lib.rmgr_ssim_hip_get_abi_version() == 6 and "#define RMGR_SSIM_HIP_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header)
    for name in ("enqueue_ssim3h", "ssim3h_device", "enqueue_ssim3h_grad", "enqueue_ssim3h_map_grad"):
        assert callable(getattr(ssim_amd.Context, name)), name
    for name in ("compute_ssim3h", "compute_ssim3h_batch", "make_params3h"):
        assert callable(getattr(ssim_amd, name)), name


# ---- the C ABI's validation (no device needed) ----

def _params(a, b, n=1, **over):
    ps = (ssim_amd.Params3H * n)()
    d, h, w = a.shape
    for i in range(n):
        ps[i] = ssim_amd.make_params3h(w, h, d, a.ctypes.data, (1, w, w * h), b.ctypes.data, (1, w, w * h))
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _grads(a, n=1):
    gs = (ssim_amd.Grad3H * n)()
    for i in range(n):
        gs[i] = ssim_amd.Grad3H(a.ctypes.data, 1, a.shape[2], a.shape[2] * a.shape[1])
    return gs


def _maps(k, n=1, strides=None):
    ms = (ssim_amd.GradOut3F * n)()
    for i in range(n):
        ms[i] = ssim_amd.GradOut3F(k.ctypes.data, *((1, k.shape[2], k.shape[2] * k.shape[1]) if strides is None else strides))
    return ms


@pytest.mark.parametrize("entry", ["enqueue", "device", "host", "grad", "map_grad"])
def test_every_einval_comes_before_the_device(lib, entry):
    shape = (6, 20, 30)
    a, b, ga = np.zeros(shape, np.uint16), np.zeros(shape, np.uint16), np.zeros(shape, np.uint16)
    k, m32 = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    out = (ctypes.c_double * 4)()
    fake_ctx = ctypes.c_void_p(1)                                              # never dereferenced
    E = errno.EINVAL
    f = getattr(lib, FNS[["enqueue", "device", "host", "grad", "map_grad"].index(entry)])
    is_grad = entry in ("grad", "map_grad")

    def rc(count=1, params=0, st=F16, r=1.0, ctx=fake_ctx, out_=0, grads=None, maps=0):
        n = max(count, 1)
        ps = _params(a, b, n) if params == 0 else params
        o = ctypes.cast(out, ctypes.c_void_p) if out_ == 0 else out_
        if entry == "grad":
            ga_, gb_ = (_grads(ga, n), None) if grads is None else grads
            return f(ctx, count, ps, st, r, o, ga_, gb_)
        if entry == "map_grad":
            ga_, gb_ = (_grads(ga, n), None) if grads is None else grads
            return f(ctx, count, ps, st, r, _maps(k, n) if maps == 0 else maps, ga_, gb_)
        if entry in ("device", "host"):
            o = ctypes.cast(o, ctypes.POINTER(ctypes.c_float)) if o is not None else None
        return f(ctx, count, ps, st, r, o)
    # everything ssim3f refuses
    assert rc(count=0) == E
    assert rc(params=None) == E
    if entry != "map_grad":
        assert rc(out_=None) == E                                              # sumsDevice / ssim / gradOutDevice NULL
    for dim in ("width", "height", "depth"):
        assert rc(params=_params(a, b, **{dim: 0})) == E
        assert rc(params=_params(a, b, **{dim: 0x7FFF0001})) == E              # above the kernels' limit
        two = _params(a, b, 2)
        setattr(two[1], dim, getattr(two[1], dim) - 1)
        assert rc(count=2, params=two) == E                                    # sizes differ
    assert rc(params=_params(a, b, width=0x7FFF0000, height=0x7FFF0000)) == E   # more than 2^24 - 1 tiles
    bad = _params(a, b)
    bad[0].imgA.topLeft = None
    assert rc(params=bad) == E
    bad = _params(a, b, 2)
    bad[1].imgB.topLeft = None
    assert rc(count=2, params=bad) == E
    for r in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert rc(r=r) == E
    # samples: an odd byte address is refused, a 2-byte aligned one is enough (valid but for the context: nothing was dereferenced)
    for img in ("imgA", "imgB"):
        bad = _params(a, b, 2)
        getattr(bad[1], img).topLeft = a.ctypes.data + 1
        assert rc(count=2, params=bad) == E
        ok = _params(a, b)
        getattr(ok[0], img).topLeft = a.ctypes.data + 2
        if entry != "host":
            assert rc(params=ok, ctx=None) == E
    # the map stays 4-byte aligned
    for off in (1, 2, 3):
        assert rc(params=_params(a, b, ssimMap=m32.ctypes.data + off)) == E
    # a sampleType that is neither constant
    for st in (2, 3, 0xFFFFFFFF):
        assert rc(st=st) == E
        assert rc(st=st, ctx=None) == E
    assert rc(st=BF16, r=float("nan")) == E
    if entry != "host":
        assert rc(ctx=None) == E and rc(ctx=None, st=BF16, r=255.0) == E       # the entry needs a context
    if is_grad:
        assert rc(grads=(None, None)) == E                                     # both gradient arrays NULL
        g = _grads(ga, 2)
        g[1].topLeft = None
        assert rc(count=2, grads=(g, None)) == E and rc(count=2, grads=(None, g)) == E
        for off in (1, 3):
            g = _grads(ga)
            g[0].topLeft = ga.ctypes.data + off                                # an odd byte address
            assert rc(grads=(g, None)) == E and rc(grads=(_grads(ga), g)) == E
        g = _grads(ga)
        g[0].topLeft = ga.ctypes.data + 2                                      # 2-byte aligned: valid but for the context
        assert rc(grads=(g, None), ctx=None) == E
    if entry == "map_grad":
        assert rc(maps=None) == E
        ms = _maps(k, 2)
        ms[1].topLeft = None
        assert rc(count=2, maps=ms) == E
        for off in (1, 2, 3):                                                  # gMap stays 4-byte aligned
            ms = _maps(k)
            ms[0].topLeft = k.ctypes.data + off
            assert rc(maps=ms) == E
        assert rc(maps=_maps(k, strides=(0, 0, 0)), ctx=None) == E


def test_host_entry_without_a_device_is_enodev(lib):
    a = np.full((4, 8, 8), 0.25, np.float16)
    if ssim_amd.device_count() > 0:
        v, m = ssim_amd.compute_ssim3h(a, a, 1.0, want_map=True)
        assert abs(float(v) - 1.0) < 1e-6 and m.shape == a.shape
        return
    with pytest.raises(ssim_amd.SsimError) as e:
        ssim_amd.compute_ssim3h(a, a, 1.0)
    assert e.value.errno == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError) as e:
        ssim_amd.compute_ssim3h_batch([(a.view(np.uint16), a.view(np.uint16))], 1.0, sample_type="bfloat16")
    assert e.value.errno == errno.ENODEV
    handle = ctypes.c_void_p()
    assert lib.rmgr_ssim_hip_create(ctypes.byref(handle), 0, None) == errno.ENODEV and not handle


def test_strides_of_views_are_taken_in_samples():
    from ssim_amd import api
    p = ssim_amd.make_params3h(30, 20, 6, 1000, (1, 30, 600), 2000, (-2, 60, -1200), 3000, (2, 60, 1200))
    assert (p.width, p.height, p.depth) == (30, 20, 6)
    assert (p.imgA.topLeft, p.imgA.step, p.imgA.stride, p.imgA.sliceStride) == (1000, 1, 30, 600)
    assert (p.imgB.topLeft, p.imgB.step, p.imgB.stride, p.imgB.sliceStride) == (2000, -2, 60, -1200)
    assert (p.ssimMap, p.ssimStep, p.ssimStride, p.ssimSliceStride) == (3000, 2, 60, 1200)
    p = ssim_amd.make_params3h(30, 20, 6, 1000, (1, 30, 600), 2000, (1, 30, 600))
    assert (p.ssimMap, p.ssimStep, p.ssimStride, p.ssimSliceStride) == (None, 1, 30, 600)
    base = np.arange(6 * 20 * 60, dtype=np.uint16).reshape(6, 20, 60)
    views = {"negative": base[::-1, ::-1, ::-1], "step 2": base[:, :, 1::2], "permuted": base.transpose(2, 0, 1), "odd offset": base[:, :, 1:]}
    for what, v in views.items():
        a, code = api._h_volume(v, "bfloat16")
        assert code == BF16 and a.ctypes.data == v.ctypes.data, what           # the view itself, not a copy
        d, h, w = a.shape
        q = api._params3h_of(a, a)
        for z, y, x in ((0, 0, 0), (d - 1, h - 1, w - 1), (1, 2, 3)):
            at = q.imgA.topLeft + 2 * (x * q.imgA.step + y * q.imgA.stride + z * q.imgA.sliceStride)
            assert at == v[z:, y:, x:].ctypes.data and (q.width, q.height, q.depth) == (w, h, d), (what, z, y, x)
    # float16 arrays select float16; uint16 arrays need a sample type; a float16 array is never bfloat16
    assert api._h_volume(base.view(np.float16), None)[1] == F16
    with pytest.raises(ValueError):
        api._h_volume(base, None)
    with pytest.raises(TypeError):
        api._h_volume(base.view(np.float16), "bfloat16")
    with pytest.raises(TypeError):
        api._h_volume(base.astype(np.float32), None)
    with pytest.raises(TypeError):
        api._h_volume(base[0], "float16")
    with pytest.raises(ValueError):
        ssim_amd.compute_ssim3h(base, base[:, :, 1:], 1.0, sample_type="float16")


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 1, 8, 16, 16)
    for fn, name in ((torch_ops.ssim3d_amp, "ssim3d_amp"), (torch_ops.ssim3d_map_amp, "ssim3d_map_amp")):
        with pytest.raises(ValueError, match="^%s: .*GPU" % name):
            fn(x, x)                                                           # float32 CPU tensors: what ssim3d raises
        with pytest.raises(TypeError, match="^%s: " % name):
            fn(x.double(), x.double())
        for t in (x.half(), x.bfloat16()):
            with pytest.raises(TypeError, match="^%s: .*GPU only" % name):
                fn(t, t)                                                       # 16-bit CPU tensors
            for pair in ((x, t), (t, x), (x.half(), x.bfloat16())):
                with pytest.raises(TypeError, match="^%s: two float32, two float16 or two bfloat16" % name):
                    fn(*pair)                                                  # a mixed pair
        with pytest.raises(TypeError):
            fn(x.numpy(), x.numpy())
        with pytest.raises(ValueError, match="^%s: " % name):
            fn(x, torch.zeros(2, 1, 8, 16, 15))
        with pytest.raises(ValueError, match="D, H, W"):
            fn(torch.zeros(16, 16), torch.zeros(16, 16))
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 0, 4, 4), torch.zeros(2, 0, 4, 4))
        for r in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                fn(x, x, r)
    # the float32-only functions keep their refusal
    for t in (x.half(), x.bfloat16()):
        with pytest.raises(TypeError, match="^ssim3d: .*float32 for now"):
            torch_ops.ssim3d(t, t)
        with pytest.raises(TypeError, match="^ssim3d_map: .*float32 for now"):
            torch_ops.ssim3d_map(t, t)
        with pytest.raises(TypeError, match="GPU only"):
            torch_ops.SSIM3DLoss()(t, t)
    with pytest.raises(ValueError, match="GPU"):
        torch_ops.SSIM3DLoss()(x, x)


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; assert 'torch' not in sys.modules; "
                        "assert callable(ssim_amd.torch_ops.ssim3d_amp) and callable(ssim_amd.torch_ops.ssim3d_map_amp)" % ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


WALK_KERNELS, MAP_WALK_KERNELS, ADJOINT_KERNELS = 2 * 4, 2 * 3, 2 * 3        # per encoding: value / dA / dB / both; dA / dB / both; dA / dB / both


def test_kernels_never_spill_and_keep_the_budgets_of_ssim3f():
    """Build-time guard, as tests/test_ssim3f_cpu.py has for ssim3f_kernels.hip.  plan3f and ssim3f_max_count are used unchanged and assume
    four workgroups per CU: the walks at most 112 VGPRs, at least 4 waves per SIMD and at most 17504 B of LDS, the adjoint walks at most
    168 VGPRs, at least 3 waves and at most 17472 B, no scratch anywhere; exactly 20 kernels (the reduction is ssim3f_kernels.hip's)."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "ssim3h_kernels.hip")
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
    walk = {k: v for k, v in kernels.items() if "ssim3h_walk" in k}
    mapwalk = {k: v for k, v in kernels.items() if "ssim3h_mapwalk" in k}
    adjoint = {k: v for k, v in kernels.items() if "ssim3h_adjoint" in k}
    assert (len(walk), len(mapwalk), len(adjoint)) == (WALK_KERNELS, MAP_WALK_KERNELS, ADJOINT_KERNELS), sorted(kernels)
    assert len(kernels) == 20, sorted(kernels)
    for k, v in sorted(kernels.items()):
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in list(walk.items()) + list(mapwalk.items()):
        assert v["VGPRs"] <= 112 and v["Occupancy"] >= 4 and v["LDS"] <= 17504, (k, v)
    for k, v in adjoint.items():
        assert v["VGPRs"] <= 168 and v["Occupancy"] >= 3 and v["LDS"] <= 17472, (k, v)


def test_stored_golden_volumes_meet_the_input_condition_of_the_float64_comparison(manifest):
    """tests/test_gpu_ssim3h.py holds value, map and sums of these volumes to the float64 model at ssim3f_model.tolerances(), twice what
    the fp32 emulation of the kernels leaves on the float32 golden volumes.  Rounding the samples into 16 bits changes the volumes (bfloat16
    keeps 8 significant bits), so the margin is checked here, not assumed: on every case the emulation stays within HALF of the
    tolerances -- the EMU_* figures themselves -- per voxel and globally.  Measured: per voxel 5.13e-4 (bbb255x63_q50_ch1 raw, either
    encoding; half the bound is 5.3e-4), global 1.76e-6 (bbb257x65_q50_ch1 unit, float16; 4.8e-6)."""
    px_tol, g_tol, _, _ = S.tolerances()
    cases = IN.golden_cases(manifest)
    assert len(cases) == 6 and set(c[1] for c in cases) == set(HM.ENCODINGS)
    worst = [0.0, 0.0]
    for i, (what, enc, ua, ub, r) in enumerate(cases):
        a, b = HM.widen(ua, enc), HM.widen(ub, enc)
        assert HM.same(HM.round_to(a, enc), ua, enc) and not np.array_equal(ua, ub)
        gv, gm = IN.golden_model(manifest, i)
        ev, em = S.emulate_fp32(a, b, r)
        px, gl = float(np.abs(em - gm).max()), abs(ev - gv)
        print("%s: emulation per voxel %.3g (half the bound: %.3g), global %.3g (%.3g)" % (what, px, px_tol / 2, gl, g_tol / 2))
        assert px <= px_tol / 2 and gl <= g_tol / 2, (what, px, gl)
        worst = [max(worst[0], px), max(worst[1], gl)]
    print("largest emulated figures: per voxel %.3g, global %.3g" % tuple(worst))
