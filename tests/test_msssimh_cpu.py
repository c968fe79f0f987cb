"""CPU: multi-scale SSIM of float16 / bfloat16 samples and its gradient -- the boundaries of rmgr_ssim_hip_*_msssimh*
(include/rmgr/ssim-hip.h).

  * the entry points are exported, every EINVAL of the msssimf entries and of the ssimh entries comes before the device, a valid call
    without a device is ENODEV, the binding and ssim_amd.torch_ops refuse what they document before any GPU call;
  * scale 0's kernels never spill and keep the budgets tests/test_msssimf_cpu.py sets for the same choreography.
"""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import ssim_amd
from conftest import ROOT

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_msssimh", "rmgr_ssim_hip_compute_msssimh_device", "rmgr_ssim_hip_compute_msssimh_host",
                "rmgr_ssim_hip_enqueue_msssimh_grad")


def _params(a, b, n=1, **over):
    ps = (ssim_amd.Params16 * n)()
    h, w = a.shape
    for i in range(n):
        ps[i] = ssim_amd.make_params16(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w)
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _grads(a, n=1):
    gs = (ssim_amd.GradH * n)()
    for i in range(n):
        gs[i] = ssim_amd.GradH(a.ctypes.data, 1, a.shape[1])
    return gs


def _weights(w):
    return None if w is None else (ctypes.c_double * len(w))(*w)


def test_entry_points_are_exported(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS
    for name in ("compute_msssimh", "compute_msssimh_batch"):
        assert hasattr(ssim_amd, name)
    for name in ("msssimh_device", "enqueue_msssimh", "enqueue_msssimh_grad"):
        assert hasattr(ssim_amd.Context, name)
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(rmgr_ssim_hip_Context\* ctx" % name, header), name
    assert lib.rmgr_ssim_hip_get_abi_version() == 6                            # additions only


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    a = np.zeros((20, 30), np.uint16)
    b = np.zeros((20, 30), np.uint16)
    ga = np.zeros((20, 30), np.uint16)
    grad, enq = fn.endswith("_grad"), fn.endswith("enqueue_msssimh")
    fake = ctypes.c_void_p(16)                                                                          # never dereferenced
    fake_ctx = None if fn.endswith("_host") else ctypes.c_void_p(1)                                     # never dereferenced
    out = fake if (grad or enq) else (ctypes.c_float * 4)()
    E = errno.EINVAL
    f = getattr(lib, fn)

    def rc(count=1, params=None, t=ssim_amd.SAMPLE_BF16, r=1.0, scales=5, w=None, o=out, ctx=fake_ctx, grads=None, means=fake):
        ps = _params(a, b, max(count, 1)) if params is None else params
        if grad:
            ga_, gb_ = (_grads(ga, max(count, 1)), None) if grads is None else grads
            return f(ctx, count, ps, t, r, scales, _weights(w), means, o, ga_, gb_)
        if enq:
            return f(ctx, count, ps, t, r, scales, _weights(w), o, means)
        return f(ctx, count, ps, t, r, scales, _weights(w), o, None)
    assert rc(count=0) == E
    if grad:
        assert f(fake_ctx, 1, None, 0, 1.0, 5, None, fake, out, _grads(ga), None) == E                   # params NULL
    else:
        assert f(fake_ctx, 1, None, 0, 1.0, 5, None, out, fake if enq else None) == E
    assert rc(o=None) == E                                                     # msssim / valuesDevice / gradOutDevice NULL
    if grad or enq:
        assert rc(means=None) == E                                             # scaleMeansDevice NULL
    for t in (2, 3, 16, 0xFFFFFFFF):
        assert rc(t=t) == E                                                    # neither of the two sample types
    assert rc(params=_params(a, b, width=0)) == E
    assert rc(params=_params(a, b, height=0)) == E
    assert rc(params=_params(a, b, width=0x7FFF0001)) == E                     # above the kernels' limit
    two = _params(a, b, 2)
    two[1].width = 29
    assert rc(count=2, params=two) == E                                        # sizes differ
    two = _params(a, b, 2)
    two[1].height = 19
    assert rc(count=2, params=two) == E
    bad = _params(a, b)
    bad[0].imgA.topLeft = None
    assert rc(params=bad) == E
    bad = _params(a, b, 2)
    bad[1].imgB.topLeft = None
    assert rc(count=2, params=bad) == E
    for off in (1, 3):
        bad = _params(a, b)
        bad[0].imgA.topLeft = a.ctypes.data + off                              # not 2-byte aligned
        assert rc(params=bad) == E
        bad = _params(a, b, 2)
        bad[1].imgB.topLeft = b.ctypes.data + off
        assert rc(count=2, params=bad) == E
    for t in (ssim_amd.SAMPLE_F16, ssim_amd.SAMPLE_BF16):
        for r in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
            assert rc(t=t, r=r) == E
    # the multi-scale rules: scales, weights, no map
    for scales in (0, 9, 100):
        assert rc(scales=scales, w=[0.1] * max(scales, 1)) == E
    for scales in (1, 4, 6, 8):
        assert rc(scales=scales, w=None) == E                                  # NULL weights are Wang's five
    for w in ([0.2, -0.1, 0.9], [0.2, float("nan"), 0.8], [float("inf"), 0.5, 0.5], [0.2, 0.3, float("-inf")]):
        assert rc(scales=3, w=w) == E
    m = np.zeros((20, 30), np.float32)
    bad = _params(a, b, 2)
    bad[1].ssimMap = m.ctypes.data
    assert rc(count=2, params=bad) == E                                        # a map
    if not fn.endswith("_host"):
        assert rc(ctx=None) == E                                               # these entries need a context
        assert rc(ctx=None, t=ssim_amd.SAMPLE_F16, scales=3, w=[0.2, 0.3, 0.5], r=255.0) == E
    if grad:
        assert rc(grads=(None, None)) == E                                     # both gradient arrays NULL
        g = _grads(ga, 2)
        g[1].topLeft = None
        assert rc(count=2, grads=(g, None)) == E and rc(count=2, grads=(None, g)) == E
        g = _grads(ga)
        g[0].topLeft = ga.ctypes.data + 1
        assert rc(grads=(g, None)) == E and rc(grads=(_grads(ga), g)) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    if ssim_amd.device_count() > 0:
        v = ssim_amd.compute_msssimh(np.full((8, 8), 0.25, np.float16), np.full((8, 8), 0.25, np.float16), 1.0)
        assert abs(float(v) - 1.0) < 1e-6
        return
    a = np.zeros((21, 31), np.uint16)
    out = (ctypes.c_float * 1)()
    for t in (ssim_amd.SAMPLE_F16, ssim_amd.SAMPLE_BF16):
        for r, scales, w in ((1.0, 5, None), (255.0, 1, [1.0]), (1000.0, 8, [0.125] * 8), (1.0, 3, [0.0, 0.0, 1.0])):
            assert lib.rmgr_ssim_hip_compute_msssimh_host(None, 1, _params(a, a), t, r, scales, _weights(w), out, None) == errno.ENODEV
    store = np.zeros(21 * 31 + 2, np.uint16)
    odd = store[(1 if store.ctypes.data % 4 == 0 else 2):][:21 * 31].reshape(21, 31)
    assert odd.ctypes.data % 4 == 2                                            # 2-byte but not 4-byte aligned: a valid pointer
    assert lib.rmgr_ssim_hip_compute_msssimh_host(None, 1, _params(odd, odd), ssim_amd.SAMPLE_BF16, 1.0, 5, None, out, None) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssimh(a.view(np.float16), a.view(np.float16), 1.0)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssimh_batch([(a, a), (a, a)], 1.0, sample_type="bfloat16", per_scale=True)


def test_the_binding_refuses_what_compute_ssimh_refuses():
    h16, u16 = np.zeros((8, 8), np.float16), np.zeros((8, 8), np.uint16)
    with pytest.raises(ValueError):
        ssim_amd.compute_msssimh(u16, u16, 1.0)                                # uint16 needs a sample type
    with pytest.raises(ValueError):
        ssim_amd.compute_msssimh(u16, u16, 1.0, sample_type="float32")
    with pytest.raises(ValueError):
        ssim_amd.compute_msssimh(u16, u16, 1.0, sample_type=2)
    with pytest.raises(TypeError):
        ssim_amd.compute_msssimh(h16, h16, 1.0, sample_type="bfloat16")         # numpy float16 is float16
    with pytest.raises(TypeError):
        ssim_amd.compute_msssimh(h16.astype(np.float32), h16.astype(np.float32), 1.0)
    with pytest.raises(TypeError):
        ssim_amd.compute_msssimh(u16.astype(np.int16), u16.astype(np.int16), 1.0, sample_type="bfloat16")
    with pytest.raises(ValueError):
        ssim_amd.compute_msssimh(h16, u16, 1.0)                                # one float16, one untyped
    with pytest.raises(TypeError):
        ssim_amd.compute_msssimh(u16, h16, 1.0, sample_type="bfloat16")         # one bfloat16, one float16
    with pytest.raises(ValueError):
        ssim_amd.compute_msssimh(h16, np.zeros((8, 9), np.float16), 1.0)
    with pytest.raises(TypeError):
        ssim_amd.compute_msssimh(h16[0], h16[0], 1.0)                          # not H x W
    with pytest.raises(ValueError):
        ssim_amd.compute_msssimh_batch([(u16, u16)], 1.0)
    with pytest.raises(TypeError):
        ssim_amd.compute_msssimh_batch([(h16, h16), (u16, u16)], 1.0, sample_type="bfloat16")


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 3, 16, 16)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="GPU only"):
            torch_ops.ms_ssim_amp(x.to(dt), x.to(dt))                          # 16-bit tensors are taken on a GPU only
        with pytest.raises(TypeError, match="GPU only"):
            torch_ops.MSSSIMLoss()(x.to(dt), x.to(dt))
        with pytest.raises(TypeError, match="ms_ssim_amp"):
            torch_ops.ms_ssim(x.to(dt), x.to(dt))                              # ms_ssim itself stays float32-only and says who is not
        with pytest.raises(TypeError):
            torch_ops.ms_ssim_amp(x, x.to(dt))                                 # mixed
        with pytest.raises(TypeError):
            torch_ops.ms_ssim_amp(x.to(dt), x)
    with pytest.raises(TypeError):
        torch_ops.ms_ssim_amp(x.half(), x.bfloat16())
    for f in (torch_ops.ms_ssim_amp, torch_ops.MSSSIMLoss()):
        with pytest.raises(ValueError):
            f(x, x)                                                            # float32 CPU tensors keep their ValueError
    for dt in (torch.float64, torch.int16, torch.uint8):
        with pytest.raises(TypeError):
            torch_ops.ms_ssim_amp(x.to(dt), x.to(dt))
    with pytest.raises(TypeError):
        torch_ops.ms_ssim_amp(x.numpy(), x.numpy())
    # scales and weights are checked where the loss is made, whatever the dtype it will see
    for kw in (dict(scales=0), dict(scales=9, weights=[0.1] * 9), dict(scales=4), dict(scales=3, weights=[0.5, 0.5]),
               dict(scales=2, weights=[0.5, -0.5]), dict(scales=2, weights=[0.5, float("nan")])):
        with pytest.raises(ValueError):
            torch_ops.MSSSIMLoss(**kw)
    with pytest.raises(TypeError):
        torch_ops.MSSSIMLoss(scales=2.0, weights=[0.5, 0.5])


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; "
                        "assert hasattr(ssim_amd, 'compute_msssimh') and 'torch' not in sys.modules" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_scale_0_kernels_never_spill_and_keep_the_float_budgets():
    """Build-time guard from the compiler's remarks, with the command line and the budgets of tests/test_msssimf_cpu.py for the same
    choreography: nothing spills; the strip kernels keep three waves per SIMD (at most 168 VGPRs, LDS for 12 waves per CU); the gradient
    kernels two workgroups of 256 lanes per CU (at most 128 VGPRs, at most 64 KiB of LDS per workgroup).  18 kernels, two encodings x (2
    strip forms, the pyramid step, 6 gradient forms: cs / ssim x A, B, both)."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "msssimh_kernels.hip")
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
    strip = {k: v for k, v in kernels.items() if "msssimh_strip" in k}
    down = {k: v for k, v in kernels.items() if "msssimh_down" in k}
    grad = {k: v for k, v in kernels.items() if "msssimh_grad" in k}
    assert len(strip) == 4 and len(down) == 2 and len(grad) == 12 and len(kernels) == 18, sorted(kernels)
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in strip.items():
        assert v["VGPRs"] <= 168 and v["Occupancy"] >= 3 and v["LDS"] <= 13312, (k, v)
    for k, v in grad.items():
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 2 and v["LDS"] <= 65536, (k, v)
    print("\n".join("%s %s" % (k, v) for k, v in sorted(kernels.items())))
