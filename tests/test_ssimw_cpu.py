"""CPU: the gradient of the SSIM map for a per-pixel upstream gradient -- the definition and its boundaries (include/rmgr/ssim-hip.h,
rmgr_ssim_hip_enqueue_ssimf_map_grad / _ssimh_map_grad, ssim_amd.torch_ops.ssim_map).

  * the float64 model (tests/ssimw_model.py) is the derivative of sum_p gmap(p) ssim(p) (central differences, corners, edges, a crop
    narrower than the window's half width and a 1 x 1 image), and with a constant plane it is ssimf_model.grad;
  * the fp32 emulation of the kernel reproduces ssimf_model.emulate_fp32 bit for bit on the constant plane and stays inside the bounds
    tests/test_gpu_ssimw.py asserts;
  * the entry points are exported, every EINVAL comes before the device, a valid call without a device is ENODEV, and
    ssim_amd.torch_ops.ssim_map refuses what it documents before any GPU call;
  * the new kernels keep the gradient kernel's budget and never spill.
"""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import ssimf_model as M
import ssimw_model as MW
import ssim_amd
from conftest import ROOT, image_entries, load_pair
from test_ssimf_cpu import _fd_points

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_ssimf_map_grad", "rmgr_ssim_hip_enqueue_ssimh_map_grad")

# the crops of test_ssimf_cpu.py::test_gradient_is_the_derivative_of_the_mean
CROPS = (("einstein_jpg", (0, 0, 40, 48)), ("einstein_blur", (100, 60, 40, 48)), ("bbb257x65_q50_ch1", (25, 209, 40, 48)),
         ("einstein_contrast", (216, 208, 40, 48)), ("einstein_jpg", (30, 30, 20, 4)), ("einstein_blur", (7, 9, 3, 5)),
         ("einstein_jpg", (50, 50, 1, 1)))


def _crops(manifest):
    for n, (y0, x0, h, w) in CROPS:
        a, b = load_pair(manifest[n])
        yield n, a[y0:y0 + h, x0:x0 + w] / 255.0, b[y0:y0 + h, x0:x0 + w] / 255.0


def test_gradient_is_the_derivative_of_the_weighted_sum(manifest):
    """Central differences of sum_p gmap(p) ssim(p) of the model's own map, at steps 1e-5 and 5e-6 (range 1), agree with grad_map()
    within 1e-7 of the plane's largest gradient magnitude -- the rule of test_ssimf_cpu.py's derivative test -- for a seeded
    standard-normal gmap and a one-hot gmap at a corner."""
    rng = np.random.default_rng(5)
    wrng = np.random.default_rng(17)
    for n, a, b in _crops(manifest):
        h, w = a.shape
        corner = np.zeros((h, w))
        corner[h - 1, 0] = 1.0
        for what, gmap in (("normal", wrng.standard_normal((h, w))), ("corner", corner)):
            ga, gb = MW.grad_map(a, b, 1.0, gmap)
            for which, gr in ((0, ga), (1, gb)):
                scale = np.abs(gr).max()
                assert scale > 0
                for eps in (1e-5, 5e-6):
                    for (y, x) in _fd_points(h, w, rng):
                        p, m = [a.copy(), b.copy()], [a.copy(), b.copy()]
                        p[which][y, x] += eps
                        m[which][y, x] -= eps
                        fd = float(np.sum(gmap * (M.ssim_map(p[0], p[1], 1.0) - M.ssim_map(m[0], m[1], 1.0)))) / (2 * eps)
                        assert abs(fd - gr[y, x]) <= 1e-7 * scale, (n, what, a.shape, which, y, x, eps, fd, gr[y, x])


def test_constant_plane_is_the_gradient_of_the_mean(manifest):
    for n, a, b in _crops(manifest):
        h, w = a.shape
        for g_out in (-0.75, 2.5):
            want = M.grad(a, b, 1.0, g_out)
            got = MW.grad_map(a, b, 1.0, np.full((h, w), g_out / (float(w) * float(h))))
            for g, wt in zip(got, want):
                assert np.abs(g - wt).max() <= 1e-15 * np.abs(wt).max(), (n, g_out)


def test_emulation_with_the_constant_plane_is_the_ssimf_emulation_bit_for_bit(manifest):
    for n in ("bbb257x65_q50_ch1", "bbb255x63_q00_ch0", "einstein_blur", "einstein_einstein"):
        a, b = load_pair(manifest[n])
        for form, fa, fb, r in M.forms(a, b):
            for g_out in (-0.75, 1.0):
                _, _, ea, eb = M.emulate_fp32(fa, fb, r, g_out)
                wa, wb = MW.emulate_fp32_map_grad(fa, fb, r, MW.constant_plane(g_out, *fa.shape))
                assert np.array_equal(wa.view(np.uint32), ea.view(np.uint32)) and np.array_equal(wb.view(np.uint32), eb.view(np.uint32)), (n, form, g_out)
    for n, a, b in _crops(manifest):                    # down to 1 x 1
        fa, fb = a.astype(np.float32), b.astype(np.float32)
        _, _, ea, eb = M.emulate_fp32(fa, fb, 1.0, -0.75)
        wa, wb = MW.emulate_fp32_map_grad(fa, fb, 1.0, MW.constant_plane(-0.75, *fa.shape))
        assert np.array_equal(wa.view(np.uint32), ea.view(np.uint32)) and np.array_equal(wb.view(np.uint32), eb.view(np.uint32)), (n, fa.shape)


def test_fp32_emulation_is_inside_the_gpu_bounds(manifest):
    """emulate_fp32_map_grad against grad_map on every golden pair in the three forms of ssimf_model.forms with the three weight planes
    of ssimw_model.weight_planes, every pixel, both gradients.  Measured: 1.06e-4 of the plane's largest float64 gradient magnitude
    (the standard-normal plane; the uniform k of ssimf measures 8.37e-5 on the same pairs); where the exact gradient is 0 -- the pair of
    identical images, and the one-hot weight at (31, 31) of einstein_impulse, whose window the impulses miss --
    max|grad| * R / max|gmap| = 8.94e-5.  tests/test_gpu_ssimw.py asserts about twice these: 2.1e-4 and 1.8e-4 -- the margin covers the
    1-ulp reciprocal and fma contraction, which the emulation does not restate."""
    worst_grad = worst_ident = 0.0
    null = []
    for i, n in enumerate(image_entries(manifest)):
        a, b = load_pair(manifest[n])
        for form, fa, fb, r in M.forms(a, b):
            for what, gmap in MW.weight_planes(*fa.shape, seed=i):
                want = MW.grad_map(fa, fb, r, gmap)
                got = MW.emulate_fp32_map_grad(fa, fb, r, gmap)
                for e, g in zip(got, want):
                    assert np.all(np.isfinite(e))
                    if MW.is_null(g, gmap, r):
                        null.append((n, what))
                        worst_ident = max(worst_ident, float(np.abs(e).max()) * r / float(np.abs(gmap).max()))
                    else:
                        assert not np.array_equal(a, b)
                        worst_grad = max(worst_grad, float(np.abs(e - g).max() / np.abs(g).max()))
    # einstein_einstein: both gradients, three forms, three weight planes; einstein_impulse under the one-hot plane: both, three forms
    assert len(null) == 24 and set(null) == {("einstein_einstein", "normal"), ("einstein_einstein", "masked"), ("einstein_einstein", "one-hot"),
                                             ("einstein_impulse", "one-hot")}, null
    print("emulation: grad %.3g null %.3g" % (worst_grad, worst_ident))
    assert worst_grad <= MW.EMU_WGRAD and worst_ident <= MW.EMU_WIDENT, (worst_grad, worst_ident)
    # pinned from below as well: a figure that moved far away means the emulation no longer restates these kernels
    assert worst_grad >= MW.EMU_WGRAD / 2 and worst_ident >= MW.EMU_WIDENT / 2, (worst_grad, worst_ident)
    for tol, emu in ((MW.WGRAD_TOL, MW.EMU_WGRAD), (MW.WIDENT_TOL, MW.EMU_WIDENT)):
        assert 1.9 <= tol / emu <= 2.2


def test_zero_weight_does_not_hide_a_nan():
    """k(p) d(p) is a plain product: a NaN sample under an all-zero gmap still gives NaN on the 21 x 21 pixels whose gradient collects a
    statistic of a window that holds it -- in the model and in the emulation."""
    rng = np.random.default_rng(3)
    a = rng.random((40, 48))
    b = np.clip(a + 0.1 * rng.standard_normal((40, 48)), 0, 1)
    a[20, 24] = np.nan
    zero = np.zeros((40, 48))
    for ga in (MW.grad_map(a, b, 1.0, zero)[0], MW.emulate_fp32_map_grad(a, b, 1.0, zero)[0]):
        bad = np.isnan(ga)
        assert bad[10:31, 14:35].all() and bad.sum() == 441 and np.all(ga[~bad] == 0)


# ---- the C ABI's validation (no device needed) ----

def _is_h(fn):
    return "ssimh" in fn


def _params(fn, a, b, n=1, **over):
    ps = ((ssim_amd.Params16 if _is_h(fn) else ssim_amd.ParamsF) * n)()
    make = ssim_amd.make_params16 if _is_h(fn) else ssim_amd.make_params_f
    h, w = a.shape
    for i in range(n):
        ps[i] = make(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w)
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _grads(fn, a, n=1):
    cls = ssim_amd.GradH if _is_h(fn) else ssim_amd.GradF
    gs = (cls * n)()
    for i in range(n):
        gs[i] = cls(a.ctypes.data, 1, a.shape[1])
    return gs


def _maps(k, n=1, step=1, stride=None):
    ms = (ssim_amd.GradOutF * n)()
    for i in range(n):
        ms[i] = ssim_amd.GradOutF(k.ctypes.data, step, k.shape[1] if stride is None else stride)
    return ms


def test_entry_points_are_exported(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS
    assert hasattr(ssim_amd, "GradOutF")
    for name in ("enqueue_ssimf_map_grad", "enqueue_ssimh_map_grad"):
        assert hasattr(ssim_amd.Context, name)
    from ssim_amd import torch_ops
    assert callable(torch_ops.ssim_map)
    assert lib.rmgr_ssim_hip_get_abi_version() == 6


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    dt = np.uint16 if _is_h(fn) else np.float32
    a, b, ga = np.zeros((20, 30), dt), np.zeros((20, 30), dt), np.zeros((20, 30), dt)
    k = np.zeros((20, 30), np.float32)
    fake_ctx = ctypes.c_void_p(1)                                              # never dereferenced
    E = errno.EINVAL
    f = getattr(lib, fn)
    none = object()

    def rc(count=1, params=None, r=1.0, maps=none, ctx=fake_ctx, grads=None, st=ssim_amd.SAMPLE_F16):
        ps = _params(fn, a, b, max(count, 1)) if params is None else params
        ms = _maps(k, max(count, 1)) if maps is none else maps
        ga_, gb_ = (_grads(fn, ga, max(count, 1)), None) if grads is None else grads
        if _is_h(fn):
            return f(ctx, count, ps, st, r, ms, ga_, gb_)
        return f(ctx, count, ps, r, ms, ga_, gb_)
    assert rc(count=0) == E
    assert (f(fake_ctx, 1, None, 0, 1.0, _maps(k), _grads(fn, ga), None) if _is_h(fn) else f(fake_ctx, 1, None, 1.0, _maps(k), _grads(fn, ga), None)) == E
    assert rc(maps=None) == E                                                  # gradOutMaps NULL
    assert rc(params=_params(fn, a, b, width=0)) == E
    assert rc(params=_params(fn, a, b, height=0)) == E
    assert rc(params=_params(fn, a, b, width=0x7FFF0001)) == E                 # above the kernels' limit
    two = _params(fn, a, b, 2)
    two[1].width = 29
    assert rc(count=2, params=two) == E                                        # sizes differ
    two = _params(fn, a, b, 2)
    two[1].height = 19
    assert rc(count=2, params=two) == E
    bad = _params(fn, a, b)
    bad[0].imgA.topLeft = None
    assert rc(params=bad) == E
    bad = _params(fn, a, b, 2)
    bad[1].imgB.topLeft = None
    assert rc(count=2, params=bad) == E
    es = a.itemsize
    for off in range(1, es):
        bad = _params(fn, a, b)
        bad[0].imgA.topLeft = a.ctypes.data + off                              # not aligned to a sample
        assert rc(params=bad) == E
        bad = _params(fn, a, b, 2)
        bad[1].imgB.topLeft = b.ctypes.data + off
        assert rc(count=2, params=bad) == E
    for r in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert rc(r=r) == E
    assert rc(ctx=None) == E                                                   # these entries need a context
    assert rc(ctx=None, r=255.0) == E
    if _is_h(fn):
        for st in (2, 3, 0xFFFFFFFF):
            assert rc(st=st) == E                                              # neither of the two sample types
        assert rc(st=ssim_amd.SAMPLE_BF16, ctx=None) == E
    assert rc(grads=(None, None)) == E                                         # both gradient arrays NULL
    g = _grads(fn, ga, 2)
    g[1].topLeft = None
    assert rc(count=2, grads=(g, None)) == E and rc(count=2, grads=(None, g)) == E
    g = _grads(fn, ga)
    g[0].topLeft = ga.ctypes.data + es // 2
    assert rc(grads=(g, None)) == E and rc(grads=(_grads(fn, ga), g)) == E
    # the gMap planes: NULL or not 4-byte aligned, in any position; steps and strides of 0 are legal and get as far as the context
    m = _maps(k, 2)
    m[1].topLeft = None
    assert rc(count=2, maps=m) == E
    for off in (1, 2, 3):
        m = _maps(k, 2)
        m[1].topLeft = k.ctypes.data + off
        assert rc(count=2, maps=m) == E
        m = _maps(k)
        m[0].topLeft = k.ctypes.data + off
        assert rc(maps=m) == E
    assert rc(maps=_maps(k, step=0, stride=0), ctx=None) == E                  # valid but for the context: nothing was dereferenced


def test_valid_call_without_a_device_fails_loudly(lib):
    """The entries take a context and nothing else (there is no _host form), and without a device no context exists: creating one is
    ENODEV, through the C ABI and through the binding.  With a device, one valid call: a single float with step = stride = 0 as gMap."""
    if ssim_amd.device_count() > 0:
        a = np.full((8, 8), 0.25, np.float32)
        with ssim_amd.Context(0) as ctx:
            da, dk, dg = ctx.upload(a), ctx.upload(np.ones(1, np.float32)), ctx.upload(np.full((8, 8), 7.0, np.float32))
            ps = (ssim_amd.ParamsF * 1)()
            ps[0] = ssim_amd.make_params_f(8, 8, da.ptr, 1, 8, da.ptr, 1, 8)
            ms, gs = (ssim_amd.GradOutF * 1)(), (ssim_amd.GradF * 1)()
            ms[0], gs[0] = ssim_amd.GradOutF(dk.ptr, 0, 0), ssim_amd.GradF(dg.ptr, 1, 8)
            ctx.enqueue_ssimf_map_grad(ps, 1, 1.0, ms, gs, None)
            ctx.synchronize()
            g = dg.download(np.float32, (8, 8))
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
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError):
        torch_ops.ssim_map(x, x)                                               # CPU tensors
    with pytest.raises(ValueError):
        torch_ops.ssim_map(x.half(), x.half())                                 # CPU tensors of a dtype it takes
    with pytest.raises(TypeError):
        torch_ops.ssim_map(x.double(), x.double())
    with pytest.raises(TypeError):
        torch_ops.ssim_map(x, x.half())                                        # mixed
    with pytest.raises(TypeError):
        torch_ops.ssim_map(x.bfloat16(), x.half())
    with pytest.raises(TypeError):
        torch_ops.ssim_map(x.to(torch.int32), x.to(torch.int32))
    with pytest.raises(TypeError):
        torch_ops.ssim_map(x.numpy(), x.numpy())
    with pytest.raises(ValueError):
        torch_ops.ssim_map(x, torch.zeros(2, 3, 16, 15))
    with pytest.raises(ValueError):
        torch_ops.ssim_map(torch.zeros(16), torch.zeros(16))
    for r in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            torch_ops.ssim_map(x, x, data_range=r)


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; assert 'torch' not in sys.modules; "
                        "assert callable(ssim_amd.torch_ops.ssim_map)" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_map_gradient_kernels_never_spill_and_keep_their_occupancy():
    """Build-time guard, as tests/test_ssimf_cpu.py has for ssimf_kernels.hip: nine kernels (float32 / float16 / bfloat16 x A / B / both),
    each within the gradient kernel's budget -- two workgroups of 256 lanes per CU (at most 128 VGPRs, at most 64 KiB of the CU's 160 KiB
    of LDS per workgroup) -- and nothing spills."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "ssimw_kernels.hip")
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
    assert len(kernels) == 9 and all("ssimw_grad_kernel" in k for k in kernels), sorted(kernels)
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 2 and v["LDS"] <= 65536, (k, v)
