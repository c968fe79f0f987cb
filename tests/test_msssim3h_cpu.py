"""CPU: multi-scale SSIM of float16 / bfloat16 volumes and its gradient -- the boundaries of rmgr_ssim_hip_*_msssim3h*
(include/rmgr/ssim-hip.h).  Sizes are W x H x D; arrays are (D, H, W); 16-bit samples travel as uint16 bit patterns.

  * the four entries are exported, declared and listed, the Python and torch names exist, the ABI version is 6;
  * every EINVAL comes before the device (tests/test_msssim3f_cpu.py's table on Params3H / Grad3H, odd addresses in place of the 4-byte
    misalignments, and the sample types that are neither constant), a valid call without a device is ENODEV;
  * ssim_amd.torch_ops refuses what it documents before any GPU call, under the new function's name, and the import stays torch-free;
  * the 28 kernels of msssim3h_kernels.hip never spill and keep the budgets of msssim3f_kernels.hip's kernels of the same role;
  * the input condition of the GPU module's golden comparison: the golden volumes as stored survive both encodings unchanged.

The sample type 0 is RMGR_SSIM_HIP_SAMPLE_F16 itself, so it is held to be VALID here (a call with it and no device is ENODEV); the
values that must be EINVAL are 2, 3, 0xFFFF and 0xFFFFFFFF.
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
import ssim_amd
from conftest import ROOT

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_msssim3h", "rmgr_ssim_hip_compute_msssim3h_device", "rmgr_ssim_hip_compute_msssim3h_host",
                "rmgr_ssim_hip_enqueue_msssim3h_grad")
HIPCC = "/opt/rocm/bin/hipcc"
F16, BF16 = ssim_amd.SAMPLE_F16, ssim_amd.SAMPLE_BF16


# ---- exports and declarations -----------------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_declared_and_listed(lib):
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS
        assert re.search(r"rmgr_int32_t %s\(" % name, header), name
    for name in ("compute_msssim3h", "compute_msssim3h_batch"):
        assert hasattr(ssim_amd, name)
    for name in ("msssim3h_device", "enqueue_msssim3h", "enqueue_msssim3h_grad"):
        assert hasattr(ssim_amd.Context, name)
    from ssim_amd import torch_ops
    assert hasattr(torch_ops, "ms_ssim3d_amp") and hasattr(torch_ops, "ms_ssim3d") and hasattr(torch_ops, "MSSSIM3DLoss")
    assert lib.rmgr_ssim_hip_get_abi_version() == 6 and ssim_amd.ABI_VERSION == 6
    assert (F16, BF16) == (0, 1) and re.search(r"#define RMGR_SSIM_HIP_SAMPLE_F16\s+0\b", header) and re.search(r"#define RMGR_SSIM_HIP_SAMPLE_BF16\s+1\b", header)


# ---- the C ABI's validation (no device needed) ------------------------------------------------------------------------------------------------

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


def _weights(w):
    return None if w is None else (ctypes.c_double * len(w))(*w)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    """The fake context and the fake device pointers are never dereferenced: an EINVAL that came after the first use of the context would
    crash."""
    a = np.zeros((6, 20, 30), np.uint16)
    b = np.zeros((6, 20, 30), np.uint16)
    ga = np.zeros((6, 20, 30), np.uint16)
    grad, enq = fn.endswith("_grad"), fn.endswith("enqueue_msssim3h")
    fake = ctypes.c_void_p(16)
    fake_ctx = None if fn.endswith("_host") else ctypes.c_void_p(1)
    out = fake if (grad or enq) else (ctypes.c_float * 4)()
    E = errno.EINVAL
    f = getattr(lib, fn)

    def rc(count=1, params=None, st=BF16, r=1.0, scales=5, w=None, o=out, ctx=fake_ctx, grads=None, means=fake):
        ps = _params(a, b, max(count, 1)) if params is None else params
        if grad:
            ga_, gb_ = (_grads(ga, max(count, 1)), None) if grads is None else grads
            return f(ctx, count, ps, st, r, scales, _weights(w), means, o, ga_, gb_)
        if enq:
            return f(ctx, count, ps, st, r, scales, _weights(w), o, means)
        return f(ctx, count, ps, st, r, scales, _weights(w), o, None)
    assert rc(count=0) == E
    if grad:
        assert f(fake_ctx, 1, None, F16, 1.0, 5, None, fake, out, _grads(ga), None) == E                 # params NULL
    else:
        assert f(fake_ctx, 1, None, F16, 1.0, 5, None, out, fake if enq else None) == E
    assert rc(o=None) == E                                                     # msssim / valuesDevice / gradOutDevice NULL
    if grad or enq:
        assert rc(means=None) == E                                             # scaleMeansDevice NULL
    for st in (2, 3, 0xFFFF, 0xFFFFFFFF):                                      # a sampleType that is neither constant
        assert rc(st=st) == E
        assert rc(st=st, scales=3, w=[0.2, 0.3, 0.5], r=255.0) == E
    for dim in ("width", "height", "depth"):
        assert rc(params=_params(a, b, **{dim: 0})) == E
        assert rc(params=_params(a, b, **{dim: 0x7FFF0001})) == E              # above the kernels' limit
        two = _params(a, b, 2)
        setattr(two[1], dim, getattr(two[1], dim) - 1)
        assert rc(count=2, params=two) == E                                    # sizes differ
    assert rc(params=_params(a, b, width=0x7FFF0000, height=0x7FFF0000)) == E  # more tiles than a launch holds
    bad = _params(a, b)
    bad[0].imgA.topLeft = None
    assert rc(params=bad) == E
    bad = _params(a, b, 2)
    bad[1].imgB.topLeft = None
    assert rc(count=2, params=bad) == E
    for st in (F16, BF16):
        for off in (1, 3, 5):
            bad = _params(a, b)
            bad[0].imgA.topLeft = a.ctypes.data + off                          # an odd address: not 2-byte aligned
            assert rc(params=bad, st=st) == E
            bad = _params(a, b, 2)
            bad[1].imgB.topLeft = b.ctypes.data + off
            assert rc(count=2, params=bad, st=st) == E
    for r in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert rc(r=r) == E
    # the multi-scale rules: scales, weights, no map
    for scales in (0, 9, 100):
        assert rc(scales=scales, w=[0.1] * max(scales, 1)) == E
    for scales in (1, 4, 6, 8):
        assert rc(scales=scales, w=None) == E                                  # NULL weights are Wang's five
    for w in ([0.2, -0.1, 0.9], [0.2, float("nan"), 0.8], [float("inf"), 0.5, 0.5], [0.2, 0.3, float("-inf")]):
        assert rc(scales=3, w=w) == E
    m = np.zeros((6, 20, 30), np.float32)
    bad = _params(a, b, 2)
    bad[1].ssimMap = m.ctypes.data
    assert rc(count=2, params=bad) == E                                        # a map
    if not fn.endswith("_host"):
        assert rc(ctx=None) == E                                               # these entries need a context
        assert rc(ctx=None, st=F16, scales=3, w=[0.2, 0.3, 0.5], r=255.0) == E
    if grad:
        assert rc(grads=(None, None)) == E                                     # both gradient arrays NULL
        g = _grads(ga, 2)
        g[1].topLeft = None
        assert rc(count=2, grads=(g, None)) == E and rc(count=2, grads=(None, g)) == E
        for off in (1, 3):
            g = _grads(ga)
            g[0].topLeft = ga.ctypes.data + off
            assert rc(grads=(g, None)) == E and rc(grads=(_grads(ga), g)) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    a = np.full((4, 8, 8), 0.25, np.float16)
    if ssim_amd.device_count() > 0:
        v = ssim_amd.compute_msssim3h(a, a, 1.0)
        assert abs(float(v) - 1.0) < 1e-6
        return
    u = np.zeros((6, 20, 30), np.uint16)
    out = (ctypes.c_float * 1)()
    # an address that is 2 mod 4 is aligned enough; the sample type 0 is float16
    for st, r, scales, w, at in ((F16, 1.0, 5, None, 0), (0, 255.0, 1, [1.0], 2), (BF16, 1000.0, 8, [0.125] * 8, 2), (1, 1.0, 3, [0.0, 0.0, 1.0], 0)):
        ps = _params(u, u)
        ps[0].imgA.topLeft = u.ctypes.data + at
        assert lib.rmgr_ssim_hip_compute_msssim3h_host(None, 1, ps, st, r, scales, _weights(w), out, None) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssim3h(a, a, 1.0)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_msssim3h_batch([(u, u), (u, u)], 1.0, sample_type="bfloat16", per_scale=True)


def test_python_binding_refuses_what_compute_ssim3h_refuses():
    a = np.zeros((4, 8, 8), np.float16)
    with pytest.raises(ValueError, match="sample_type"):
        ssim_amd.compute_msssim3h(a.view(np.uint16), a.view(np.uint16), 1.0)               # bit patterns without an encoding
    with pytest.raises(TypeError, match="bfloat16"):
        ssim_amd.compute_msssim3h(a, a, 1.0, sample_type="bfloat16")                      # a float16 array declared bfloat16
    with pytest.raises(TypeError):
        ssim_amd.compute_msssim3h(a.astype(np.float32), a.astype(np.float32), 1.0)
    with pytest.raises(ValueError, match="shapes differ"):
        ssim_amd.compute_msssim3h(a, a[:, :, 1:], 1.0)


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 3, 8, 16, 16)
    with pytest.raises(ValueError, match="^ms_ssim3d_amp: .*on a GPU"):
        torch_ops.ms_ssim3d_amp(x, x)                                          # a float32 CPU pair
    with pytest.raises(ValueError, match="^ms_ssim3d_amp: "):
        torch_ops.MSSSIM3DLoss()(x, x)
    for half in (torch.float16, torch.bfloat16):
        # a 16-bit CPU pair: taken on a GPU only, and the phrase tests/test_msssim3f_cpu.py pins on MSSSIM3DLoss
        for f in (torch_ops.ms_ssim3d_amp, torch_ops.MSSSIM3DLoss()):
            with pytest.raises(TypeError, match="^ms_ssim3d_amp: .*taken on a GPU only .*3-D multi-scale path is float32 for now"):
                f(x.to(half), x.to(half))
        # a mixed pair
        for p, q in ((x, x.to(half)), (x.to(half), x), (x.to(half), x.to(torch.bfloat16 if half is torch.float16 else torch.float16))):
            with pytest.raises(TypeError, match="^ms_ssim3d_amp: two float32, two float16 or two bfloat16"):
                torch_ops.ms_ssim3d_amp(p, q)
        # ms_ssim3d keeps its refusal, message unchanged at its start
        with pytest.raises(TypeError, match="^ms_ssim3d: the 3-D multi-scale path is float32 for now, got"):
            torch_ops.ms_ssim3d(x.to(half), x.to(half))
    with pytest.raises(TypeError, match="^ms_ssim3d_amp: "):
        torch_ops.ms_ssim3d_amp(x.double(), x.double())
    with pytest.raises(TypeError, match="^ms_ssim3d_amp: "):
        torch_ops.ms_ssim3d_amp(x.numpy(), x.numpy())
    with pytest.raises(ValueError, match="^ms_ssim3d_amp: shapes differ"):
        torch_ops.ms_ssim3d_amp(x, torch.zeros(2, 3, 8, 16, 15))
    with pytest.raises(ValueError, match="^ms_ssim3d_amp: .*D, H, W"):
        torch_ops.ms_ssim3d_amp(torch.zeros(16, 16), torch.zeros(16, 16))
    # the scales / weights errors carry the new name; they come after the tensors' own, so the tensors must pass: none can on a CPU, and
    # the helper is the one ms_ssim3d_amp calls
    for kw in (dict(scales=0), dict(scales=9, weights=[0.1] * 9), dict(scales=4), dict(scales=3, weights=[0.5, 0.5]),
               dict(scales=2, weights=[0.5, -0.5]), dict(scales=2, weights=[0.5, float("nan")]), dict(scales=2, weights=[float("inf"), 0.5])):
        with pytest.raises(ValueError, match="^ms_ssim3d_amp: "):
            torch_ops._ms_ssim3d(x, x, 1.0, kw["scales"], kw.get("weights"), "ms_ssim3d_amp")
    with pytest.raises(TypeError, match="^ms_ssim3d_amp: "):
        torch_ops._ms_ssim3d(x, x, 1.0, 2.0, [0.5, 0.5], "ms_ssim3d_amp")


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; "
                        "ssim_amd.torch_ops.MSSSIM3DLoss(scales=2, weights=(0.5, 0.5)); "
                        "assert hasattr(ssim_amd.torch_ops, 'ms_ssim3d_amp') and hasattr(ssim_amd, 'compute_msssim3h') and 'torch' not in sys.modules" % ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- budgets ------------------------------------------------------------------------------------------------------------------------------------

def test_sixteen_bit_multi_scale_volume_kernels_never_spill_and_keep_the_float32_budgets():
    """Build-time guard from the compiler's remarks, by the mechanism of tests/test_msssim3f_cpu.py and with its budgets.  28 kernels: per
    encoding 7 walks (the value walk with two sums; dA, dB, both in the cs form and in the ssim form), 6 adjoint walks (A, B, both x only
    scale / finer) and the pyramid step.  None uses scratch; every walk keeps 4 waves per SIMD or more (at most 128 VGPRs) and the
    float32 walks' LDS (17472 bytes, plus 64 for the second sum's wave totals); the one-gradient adjoints keep 4 waves or more, the
    both-gradients adjoints 3 or more (at most 168 VGPRs)."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "msssim3h_kernels.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
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
    walks = {k: v for k, v in kernels.items() if "msssim3h_walk_kernel" in k}
    adjoints = {k: v for k, v in kernels.items() if "msssim3h_adjoint_kernel" in k}
    downs = {k: v for k, v in kernels.items() if "msssim3h_down_kernel" in k}
    assert len(walks) == 14 and len(adjoints) == 12 and len(downs) == 2 and len(kernels) == 28, sorted(kernels)
    for k, v in sorted(kernels.items()):
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in walks.items():
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 4 and v["LDS"] <= 17472 + 64, (k, v)
    for k, v in adjoints.items():
        # template arguments <TYPE, WHICH, MS>: WHICH is the second
        which = int(re.search(r"msssim3h_adjoint_kernelILi\dELi(\d)ELi\dE", k).group(1))
        assert v["Occupancy"] >= (3 if which == 3 else 4) and v["VGPRs"] <= (168 if which == 3 else 128) and v["LDS"] <= 17472, (k, v)


def test_the_float32_objects_still_link_without_the_new_one():
    """msssim3f_kernels.o defines the _from launchers and needs nothing of msssim3h_kernels.o (tests/src/msssim3f_plan_probe.cpp links it
    with ssim3f_kernels.o alone); the new object's undefined ssim_hip symbols are all defined by those two."""
    objects = ["build/obj/msssim3f_kernels.o", "build/obj/ssim3f_kernels.o", "build/obj/msssim3h_kernels.o"]
    r = subprocess.run(["make", "-C", ROOT] + objects, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]

    def symbols(obj, flag):
        out = subprocess.run(["nm", "-C", flag, os.path.join(ROOT, obj)], capture_output=True, text=True, check=True).stdout
        return set(re.sub(r"\(.*", "", ln.split(None, 2 if flag == "--defined-only" else 1)[-1]) for ln in out.splitlines() if "ssim_hip::" in ln)
    defined = symbols(objects[0], "--defined-only") | symbols(objects[1], "--defined-only")
    assert "ssim_hip::launch_msssim3f_from" in defined and "ssim_hip::launch_msssim3f_grad_from" in defined
    assert not any("msssim3h" in s for s in symbols(objects[0], "--undefined-only"))
    needs = symbols(objects[2], "--undefined-only")
    assert "ssim_hip::launch_msssim3f_from" in needs and needs <= defined, needs - defined


# ---- the input condition of the golden comparison -----------------------------------------------------------------------------------------------

def test_stored_golden_volumes_survive_both_encodings(manifest):
    """tests/test_gpu_msssim3h.py holds the five golden volumes as stored (range 255) to the float64 model at msssim3f_model's bounds, which
    were measured on these very float32 volumes: integers 0 .. 255 have at most 8 significant bits, so both encodings hold them exactly."""
    for name in S.FIXTURES:
        (form, a, b, r), = S.fixture_forms(manifest, name, ("raw",))
        assert r == 255.0 and a.dtype == np.float32
        for v in (a, b):
            assert np.array_equal(v, np.round(v)) and v.min() >= 0 and v.max() <= 255
            for enc in HM.ENCODINGS:
                assert np.array_equal(HM.widen(HM.round_to(v, enc), enc).view(np.uint32), v.view(np.uint32)), (name, enc)
