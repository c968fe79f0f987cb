"""CPU: SSIM of float16 / bfloat16 samples and its gradient -- the boundaries of rmgr_ssim_hip_*_ssimh* (include/rmgr/ssim-hip.h).

  * the reference widening and rounding of tests/halfmodel.py are torch's CPU conversions, bit for bit;
  * the entry points are exported, every EINVAL comes before the device, a valid call without a device is ENODEV, the binding and
    ssim_amd.torch_ops refuse what they document before any GPU call;
  * the new kernels never spill and keep ssimf's budgets.
"""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import halfmodel as HM
import ssim_amd
from conftest import ROOT

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_ssimh", "rmgr_ssim_hip_compute_ssimh_device", "rmgr_ssim_hip_compute_ssimh_host",
                "rmgr_ssim_hip_enqueue_ssimh_grad")


# ---- the reference conversions ----

def _torch_bf16_widen(u16):
    import torch
    return torch.from_numpy(u16.view(np.int16).copy()).view(torch.bfloat16).float().numpy()


def _torch_bf16_round(f32):
    import torch
    return torch.from_numpy(f32.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _edge_floats():
    """Ties, the largest finite values, subnormals, +-0, +-Inf and NaN, as float32 bit patterns."""
    u = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7FBFFFFF,
         0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001,      # the largest finite bfloat16 and what rounds to Inf
         0x477FE000, 0x477FEFFF, 0x477FF000, 0x477FF001, 0xC77FF000,                  # 65504, and the tie to float16 Inf
         0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x00800000, 0x807FFFFF,   # float32 / bfloat16 subnormals
         0x33000000, 0x33000001, 0x32FFFFFF, 0x33800000, 0x33C00000, 0x38800000, 0x387FC000, 0x387FE000, 0x387FF000, 0xB87FF000]  # float16's
    for base in (0x3F800000, 0x3F810000, 0xBF800000, 0x40490000, 0x00010000):         # ties of both encodings: to even, both ways
        for low in (0x0FFF, 0x1000, 0x1001, 0x2FFF, 0x3000, 0x3001, 0x7FFF, 0x8000, 0x8001, 0x17FFF, 0x18000, 0x18001):
            u.append(base + low)
    return np.array(u, np.uint32).view(np.float32)


def test_bfloat16_widening_is_torchs_over_all_patterns():
    u = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got, want = HM.widen(u, HM.BF16), _torch_bf16_widen(u)
    assert HM.same_f32(got, want)
    # exact: the upper half of the float32 is the sample, the lower half is zero -- NaN and Inf included
    assert np.array_equal(got.view(np.uint32) >> 16, u) and np.all((got.view(np.uint32) & 0xFFFF) == 0)
    assert HM.same(HM.round_to(got, HM.BF16), u, HM.BF16)                       # and rounding a widened sample gives it back


def test_float16_widening_is_exact_over_all_patterns():
    import torch
    u = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = HM.widen(u, HM.F16)
    want = torch.from_numpy(u.view(np.int16).copy()).view(torch.float16).float().numpy()
    assert HM.same_f32(got, want)
    sub = HM.is_subnormal(u, HM.F16)
    assert sub.sum() == 2046 and np.all(np.abs(got[sub]) >= 2.0 ** -24) and np.all(np.abs(got[sub]).view(np.uint32) >= 0x00800000)   # float32 normals
    assert HM.same(HM.round_to(got, HM.F16), u, HM.F16)


def test_rounding_is_torchs_nearest_even():
    import torch
    rng = np.random.default_rng(2024)
    f = np.concatenate([rng.integers(0, 1 << 32, 400000, dtype=np.uint64).astype(np.uint32).view(np.float32), _edge_floats(),
                        (rng.standard_normal(100000) * 1e-5).astype(np.float32)])
    assert HM.same(HM.round_to(f, HM.BF16), _torch_bf16_round(f), HM.BF16)
    want16 = torch.from_numpy(f.copy()).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert HM.same(HM.round_to(f, HM.F16), want16, HM.F16)
    # spot values: ties go to even, the largest finite values round to Inf past their half-way point, subnormals are kept
    r = lambda bits, enc: int(HM.round_to(np.array([bits], np.uint32).view(np.float32), enc)[0])
    assert r(0x3F808000, HM.BF16) == 0x3F80 and r(0x3F818000, HM.BF16) == 0x3F82 and r(0x3F808001, HM.BF16) == 0x3F81
    assert r(0x7F7F7FFF, HM.BF16) == 0x7F7F and r(0x7F7F8000, HM.BF16) == 0x7F80 and r(0x00008001, HM.BF16) == 0x0001
    assert r(0x477FEFFF, HM.F16) == 0x7BFF and r(0x477FF000, HM.F16) == 0x7C00 and r(0x33800000, HM.F16) == 0x0001 and r(0x33000000, HM.F16) == 0
    assert HM.is_nan(np.uint16(r(0x7F800001, HM.BF16)), HM.BF16) and HM.is_nan(np.uint16(r(0xFFFFFFFF, HM.F16)), HM.F16)


# ---- the C ABI's validation (no device needed) ----

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


def test_entry_points_are_exported(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS
    for name in ("GradH", "SAMPLE_F16", "SAMPLE_BF16", "compute_ssimh", "compute_ssimh_batch"):
        assert hasattr(ssim_amd, name)
    for name in ("ssimh_device", "enqueue_ssimh", "enqueue_ssimh_grad"):
        assert hasattr(ssim_amd.Context, name)
    assert (ssim_amd.SAMPLE_F16, ssim_amd.SAMPLE_BF16) == (0, 1)
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    assert re.search(r"#define RMGR_SSIM_HIP_SAMPLE_F16\s+0\b", header) and re.search(r"#define RMGR_SSIM_HIP_SAMPLE_BF16\s+1\b", header)
    assert lib.rmgr_ssim_hip_get_abi_version() == 6                            # additions only


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    a = np.zeros((20, 30), np.uint16)
    b = np.zeros((20, 30), np.uint16)
    ga = np.zeros((20, 30), np.uint16)
    grad = fn.endswith("_grad")
    out = (ctypes.c_float * 4)() if not fn.startswith("rmgr_ssim_hip_enqueue") else ctypes.c_void_p(16)   # never dereferenced
    fake_ctx = None if fn.endswith("_host") else ctypes.c_void_p(1)                                     # never dereferenced
    E = errno.EINVAL
    f = getattr(lib, fn)

    def rc(count=1, params=None, t=ssim_amd.SAMPLE_BF16, r=1.0, o=out, ctx=fake_ctx, grads=None):
        ps = _params(a, b, max(count, 1)) if params is None else params
        if grad:
            ga_, gb_ = (_grads(ga, max(count, 1)), None) if grads is None else grads
            return f(ctx, count, ps, t, r, o, ga_, gb_)
        return f(ctx, count, ps, t, r, o)
    assert rc(count=0) == E
    assert (f(fake_ctx, 1, None, 0, 1.0, out, _grads(ga), None) if grad else f(fake_ctx, 1, None, 0, 1.0, out)) == E      # params NULL
    assert rc(o=None) == E                                                     # ssim / sumsDevice / gradOutDevice NULL
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
    if not fn.endswith("_host"):
        assert rc(ctx=None) == E                                               # these entries need a context
        assert rc(ctx=None, t=ssim_amd.SAMPLE_F16, r=255.0) == E
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
        v, _ = ssim_amd.compute_ssimh(np.full((8, 8), 0.25, np.float16), np.full((8, 8), 0.25, np.float16), 1.0)
        assert abs(float(v) - 1.0) < 1e-6
        return
    a = np.zeros((21, 31), np.uint16)
    out = (ctypes.c_float * 1)()
    for t in (ssim_amd.SAMPLE_F16, ssim_amd.SAMPLE_BF16):
        for r in (1.0, 255.0):
            assert lib.rmgr_ssim_hip_compute_ssimh_host(None, 1, _params(a, a), t, r, out) == errno.ENODEV
    store = np.zeros(21 * 31 + 2, np.uint16)
    odd = store[(1 if store.ctypes.data % 4 == 0 else 2):][:21 * 31].reshape(21, 31)
    assert odd.ctypes.data % 4 == 2                                            # 2-byte but not 4-byte aligned: a valid pointer
    assert lib.rmgr_ssim_hip_compute_ssimh_host(None, 1, _params(odd, odd), ssim_amd.SAMPLE_BF16, 1.0, out) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssimh(a.view(np.float16), a.view(np.float16), 1.0)
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssimh_batch([(a, a), (a, a)], 1.0, sample_type="bfloat16")


def test_the_binding_refuses_what_it_documents():
    h16, u16 = np.zeros((8, 8), np.float16), np.zeros((8, 8), np.uint16)
    with pytest.raises(ValueError):
        ssim_amd.compute_ssimh(u16, u16, 1.0)                                  # uint16 needs a sample type
    with pytest.raises(ValueError):
        ssim_amd.compute_ssimh(u16, u16, 1.0, sample_type="float32")
    with pytest.raises(ValueError):
        ssim_amd.compute_ssimh(u16, u16, 1.0, sample_type=2)
    with pytest.raises(TypeError):
        ssim_amd.compute_ssimh(h16, h16, 1.0, sample_type="bfloat16")           # numpy float16 is float16
    with pytest.raises(TypeError):
        ssim_amd.compute_ssimh(h16.astype(np.float32), h16.astype(np.float32), 1.0)
    with pytest.raises(TypeError):
        ssim_amd.compute_ssimh(u16.astype(np.int16), u16.astype(np.int16), 1.0, sample_type="bfloat16")
    with pytest.raises(ValueError):
        ssim_amd.compute_ssimh(h16, u16, 1.0)                                  # one float16, one untyped
    with pytest.raises(TypeError):
        ssim_amd.compute_ssimh(u16, h16, 1.0, sample_type="bfloat16")           # one bfloat16, one float16
    with pytest.raises(ValueError):
        ssim_amd.compute_ssimh(h16, np.zeros((8, 9), np.float16), 1.0)
    with pytest.raises(TypeError):
        ssim_amd.compute_ssimh(h16[0], h16[0], 1.0)                            # not H x W
    with pytest.raises(ValueError):
        ssim_amd.compute_ssimh_batch([(u16, u16)], 1.0)
    assert ssim_amd.sample_type_code("float16") == 0 and ssim_amd.sample_type_code("bfloat16") == 1 and ssim_amd.sample_type_code(1) == 1


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 3, 16, 16)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError):
            torch_ops.ssim(x.to(dt), x.to(dt))                                 # CPU tensors: there is no CPU path
        with pytest.raises(ValueError):
            torch_ops.SSIMLoss()(x.to(dt), x.to(dt))
        with pytest.raises(TypeError):
            torch_ops.ssim(x, x.to(dt))                                        # mixed
        with pytest.raises(TypeError):
            torch_ops.ssim(x.to(dt), x)
        with pytest.raises(TypeError):
            torch_ops.ms_ssim(x.to(dt), x.to(dt))                              # the multi-scale path stays float32
        with pytest.raises(TypeError):
            torch_ops.MSSSIMLoss()(x.to(dt), x.to(dt))
        with pytest.raises(ValueError):
            torch_ops.ssim(x.to(dt), torch.zeros(2, 3, 16, 15, dtype=dt))
    with pytest.raises(TypeError):
        torch_ops.ssim(x.half(), x.bfloat16())
    for dt in (torch.float64, torch.int16, torch.uint8):
        with pytest.raises(TypeError):
            torch_ops.ssim(x.to(dt), x.to(dt))


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; assert 'torch' not in sys.modules" % ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_half_kernels_never_spill_and_keep_their_occupancy():
    """Build-time guard, as tests/test_ssimf_cpu.py has for ssimf_kernels.hip, with that file's budgets: the strip kernels keep three
    waves per SIMD (at most 168 VGPRs, LDS for 12 waves per CU), the gradient kernels two workgroups of 256 lanes per CU (at most 128
    VGPRs, at most 64 KiB of LDS per workgroup), and nothing spills.  Two encodings x (five strip forms + three gradient forms) and the
    reduction: 17 kernels."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "ssimh_kernels.hip")
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
    strip = {k: v for k, v in kernels.items() if "ssimh_strip" in k}
    grad = {k: v for k, v in kernels.items() if "ssimh_grad" in k}
    assert len(strip) == 10 and len(grad) == 6 and len(kernels) == 17, sorted(kernels)     # + the reduction
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in strip.items():
        assert v["VGPRs"] <= 168 and v["Occupancy"] >= 3 and v["LDS"] <= 13312, (k, v)
    for k, v in grad.items():
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 2 and v["LDS"] <= 65536, (k, v)
    print("\n".join("%s %s" % (k, v) for k, v in sorted(kernels.items())))
