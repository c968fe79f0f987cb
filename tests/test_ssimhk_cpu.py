"""CPU: SSIM of float16 / bfloat16 planes under a caller-chosen window, its gradient and the gradient of its map -- the boundaries of the
rmgr_ssim_hip_*_ssimh_win* entries (include/rmgr/ssim-hip.h).  Sizes are W x H; arrays are (H, W); 16-bit samples travel as uint16 bit
patterns.

  * the five entry points are exported, declared and listed; the Python keywords exist;
  * every EINVAL of a window comes before the device, and so does every EINVAL of the entry without _win, under a valid window and NULL;
  * _host without a device is ENODEV;
  * ssim_amd.torch_ops: the window errors of ssim_amp and ssim_map_amp are those tests/test_ssimk_cpu.py lists, at every dtype; two
    16-bit CPU tensors with a window reach the device check ("GPU", a ValueError), not "fixed window"; ssim, ssim_map and SSIMLoss keep
    "fixed window" on them; the import stays torch-free;
  * ssimhk_kernels.hip never spills, holds 32 strip, 24 gradient and 1 reduction kernel, and keeps the budgets tests/test_ssimk_cpu.py
    asserts for the float32 kernels of the same radii;
  * the input condition of the GPU module's rounding test: under every window, the float64 model's gradient of the chosen planes,
    rounded to float16, holds subnormals at the small upstream gradient and both Inf and normal numbers at the large one.
"""
import ctypes
import errno
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import halfmodel as HM
import ssimhk_inputs as IN
import ssimk_model as K
import ssim_amd
from conftest import ROOT
from test_ssim3k_cpu import BAD_WINDOWS, GOOD_WINDOWS

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_ssimh_win", "rmgr_ssim_hip_compute_ssimh_win_device", "rmgr_ssim_hip_compute_ssimh_win_host",
                "rmgr_ssim_hip_enqueue_ssimh_win_grad", "rmgr_ssim_hip_enqueue_ssimh_win_map_grad")
F16, BF16 = ssim_amd.SAMPLE_F16, ssim_amd.SAMPLE_BF16
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "ssim_amd", "csrc")


# ---- symbols ------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_declared_and_listed(lib):
    with open(os.path.join(ROOT, "include", "rmgr", "ssim-hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS, name
        assert re.search(r"rmgr_int32_t %s\(" % name, header), name
    assert lib.rmgr_ssim_hip_get_abi_version() == 6 and "#define RMGR_SSIM_HIP_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header)


def test_python_keywords_exist_and_take_a_window_only(lib):
    for fn in (ssim_amd.compute_ssimh, ssim_amd.compute_ssimh_batch, ssim_amd.Context.ssimh_device, ssim_amd.Context.enqueue_ssimh,
               ssim_amd.Context.enqueue_ssimh_grad, ssim_amd.Context.enqueue_ssimh_map_grad):
        p = inspect.signature(fn).parameters
        assert "window" in p and p["window"].default is None and list(p)[-1] == "window", fn
    a = np.zeros((3, 4), np.float16)
    with pytest.raises(TypeError):
        ssim_amd.compute_ssimh(a, a, 1.0, window=(7, 1.5))
    with pytest.raises(TypeError):
        ssim_amd.compute_ssimh_batch([(a, a)], 1.0, window="uniform")
    ctx = ssim_amd.Context.__new__(ssim_amd.Context)           # no device, no handle: the window is refused before the library is called
    ctx.lib, ctx.handle = lib, None
    ps = (ssim_amd.Params16 * 1)()
    for call in (lambda w: ctx.ssimh_device(ps, 1, 1.0, "float16", window=w), lambda w: ctx.enqueue_ssimh(ps, 1, 1.0, "float16", 16, window=w),
                 lambda w: ctx.enqueue_ssimh_grad(ps, 1, 1.0, "bfloat16", 16, None, None, window=w),
                 lambda w: ctx.enqueue_ssimh_map_grad(ps, 1, 1.0, "bfloat16", None, None, None, window=w)):
        for w in ((7, 1.5), "uniform", 7):
            with pytest.raises(TypeError, match="ssim_amd.Window"):
                call(w)


# ---- the C ABI's validation (no device needed) -----------------------------------------------------------------------------------------

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


def _gmaps(k, n=1):
    gs = (ssim_amd.GradOutF * n)()
    for i in range(n):
        gs[i] = ssim_amd.GradOutF(k.ctypes.data, 1, k.shape[1])
    return gs


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    """The fake context and the fake device pointers are never dereferenced: an EINVAL that came after the first use of the context
    would crash.  A valid window with a NULL context is EINVAL too (the entries that need one), which shows the window passed."""
    shape = (20, 30)
    a, b, ga = np.zeros(shape, np.uint16), np.zeros(shape, np.uint16), np.zeros(shape, np.uint16)
    k = np.zeros(shape, np.float32)
    grad, mapg, host = fn.endswith("_grad"), fn.endswith("_map_grad"), fn.endswith("_host")
    out = _gmaps(k, 2) if mapg else ((ctypes.c_float * 4)() if not fn.startswith("rmgr_ssim_hip_enqueue") else ctypes.c_void_p(16))
    fake_ctx = None if host else ctypes.c_void_p(1)
    E = errno.EINVAL
    f = getattr(lib, fn)

    def win(w):
        return None if w is None else ctypes.byref(ssim_amd.Window(*w))

    def rc(count=1, params=None, st=F16, r=1.0, o=out, ctx=fake_ctx, grads=None, w=(7, 1, 0.0)):
        ps = _params(a, b, max(count, 1)) if params is None else params
        if grad:
            ga_, gb_ = (_grads(ga, max(count, 1)), None) if grads is None else grads
            return f(ctx, count, ps, st, r, win(w), o, ga_, gb_)
        return f(ctx, count, ps, st, r, win(w), o)
    # the window: a bad size (4, 13, 1, ...), a bad kind, sigma 0 / negative / NaN / Inf for a Gaussian
    for w in BAD_WINDOWS:
        for st in (F16, BF16):
            assert rc(w=w, st=st) == E, w
            assert rc(w=w, st=st, count=2) == E, w
    # sigma ignored for a box, NULL, the engine's window: valid so far -- the NULL context is what is refused
    if not host:
        for w in GOOD_WINDOWS:
            assert rc(w=w, ctx=None) == E, w
            assert rc(w=w, ctx=None, st=BF16, r=255.0) == E, w
    # every EINVAL of the entry without _win, under a valid window and under NULL
    for w in ((7, 1, 0.0), (11, 0, 2.0), None):
        assert rc(count=0, w=w) == E
        assert (f(fake_ctx, 1, None, F16, 1.0, win(w), out, _grads(ga), None) if grad else f(fake_ctx, 1, None, F16, 1.0, win(w), out)) == E
        assert rc(o=None, w=w) == E
        for dim in ("width", "height"):
            assert rc(params=_params(a, b, **{dim: 0}), w=w) == E
            assert rc(params=_params(a, b, **{dim: 0x7FFF0001}), w=w) == E
            two = _params(a, b, 2)
            setattr(two[1], dim, getattr(two[1], dim) - 1)
            assert rc(count=2, params=two, w=w) == E
        bad = _params(a, b)
        bad[0].imgA.topLeft = None
        assert rc(params=bad, w=w) == E
        bad = _params(a, b, 2)
        bad[1].imgB.topLeft = None
        assert rc(count=2, params=bad, w=w) == E
        for img in ("imgA", "imgB"):                               # an odd byte address is refused, a 2-byte aligned one is enough
            bad = _params(a, b, 2)
            getattr(bad[1], img).topLeft = a.ctypes.data + 1
            assert rc(count=2, params=bad, w=w) == E
            ok = _params(a, b)
            getattr(ok[0], img).topLeft = a.ctypes.data + 2
            if not host:
                assert rc(params=ok, ctx=None, w=w) == E
        for st in (2, 3, 0xFFFFFFFF):                              # a sampleType that is neither constant
            assert rc(st=st, w=w) == E
        for r in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
            assert rc(r=r, w=w) == E
        if grad:
            assert rc(grads=(None, None), w=w) == E
            g = _grads(ga, 2)
            g[1].topLeft = None
            assert rc(count=2, grads=(g, None), w=w) == E and rc(count=2, grads=(None, g), w=w) == E
            for off in (1, 3):
                g = _grads(ga)
                g[0].topLeft = ga.ctypes.data + off
                assert rc(grads=(g, None), w=w) == E and rc(grads=(_grads(ga), g), w=w) == E
        if mapg:
            m = _gmaps(k, 2)
            m[1].topLeft = None
            assert rc(count=2, o=m, w=w) == E
            for off in (1, 2, 3):
                m = _gmaps(k)
                m[0].topLeft = k.ctypes.data + off
                assert rc(o=m, w=w) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    win = ssim_amd.make_window(3, kind="uniform")
    a = np.full((8, 8), 0.25, np.float16)
    if ssim_amd.device_count() > 0:
        v, _ = ssim_amd.compute_ssimh(a, a, 1.0, window=win)
        assert abs(float(v) - 1.0) < 1e-6
        return
    u = np.zeros((20, 30), np.uint16)
    out = (ctypes.c_float * 1)()
    for st in (F16, BF16):
        assert lib.rmgr_ssim_hip_compute_ssimh_win_host(None, 1, _params(u, u), st, 1.0, ctypes.byref(win), out) == errno.ENODEV
        assert lib.rmgr_ssim_hip_compute_ssimh_win_host(None, 1, _params(u, u), st, 1.0, None, out) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError) as e:
        ssim_amd.compute_ssimh(a, a, 1.0, window=win)
    assert e.value.errno == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError) as e:
        ssim_amd.compute_ssimh_batch([(u, u), (u, u)], 1.0, sample_type="bfloat16", window=win)
    assert e.value.errno == errno.ENODEV


# ---- torch_ops (CPU tensors) -----------------------------------------------------------------------------------------------------------

def test_torch_ops_window_errors_come_first_at_every_dtype():
    """The lists of tests/test_ssimk_cpu.py for ssim_amp and ssim_map_amp, with float32, float16 and bfloat16 CPU tensors: a bad window
    is refused before the tensors are looked at; a valid one reaches the device check at every dtype and never says "fixed window"."""
    import torch
    from ssim_amd import torch_ops
    x32 = torch.zeros(2, 3, 16, 16)
    for x in (x32, x32.half(), x32.bfloat16()):
        for name, fn in (("ssim_amp", torch_ops.ssim_amp), ("ssim_map_amp", torch_ops.ssim_map_amp)):
            for kw in (dict(win_size=7.0), dict(win_size="7"), dict(win_size=True), dict(window=1), dict(window=None)):
                with pytest.raises(TypeError) as e:
                    fn(x, x, **kw)
                assert "fixed window" not in str(e.value), kw
            for kw in (dict(win_size=4), dict(win_size=13), dict(win_size=1), dict(win_size=-3), dict(win_sigma=0.0), dict(win_sigma=-1.0),
                       dict(win_sigma=float("nan")), dict(win_sigma=float("inf")), dict(window="box"), dict(window="Gaussian")):
                with pytest.raises(ValueError) as e:
                    fn(x, x, **kw)
                assert "GPU" not in str(e.value), kw
            for kw in (dict(win_size=7), dict(win_sigma=2.0), dict(window="uniform"), dict(win_size=3, window="uniform"),
                       dict(window="uniform", win_sigma=float("nan")), dict()):
                with pytest.raises(ValueError, match="^%s: .*GPU" % name) as e:
                    fn(x, x, **kw)
                assert "fixed window" not in str(e.value)
    # every other error is ssim's, under the function's own name
    for name, fn in (("ssim_amp", torch_ops.ssim_amp), ("ssim_map_amp", torch_ops.ssim_map_amp)):
        with pytest.raises(TypeError, match="^%s: two float32, two float16 or two bfloat16" % name):
            fn(x32, x32.half(), win_size=7)
        with pytest.raises(TypeError, match="^%s: x and y must be torch tensors" % name):
            fn(x32.numpy(), x32, win_size=7)
        with pytest.raises(ValueError, match="^%s: shapes differ" % name):
            fn(x32.half(), x32.half()[:, :, :8], win_size=7)
        with pytest.raises(ValueError, match="^%s: tensors of shape" % name):
            fn(x32[0, 0, 0], x32[0, 0, 0])


def test_the_fixed_window_refusals_stay_as_they_are():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 3, 16, 16)
    for t in (x.half(), x.bfloat16()):
        for fn in (torch_ops.ssim, torch_ops.ssim_map, lambda a, b, **kw: torch_ops.SSIMLoss(**kw)(a, b)):
            for kw in (dict(win_size=7), dict(win_sigma=2.0), dict(window="uniform"), dict(win_size=3, window="uniform")):
                with pytest.raises(TypeError, match="fixed window"):
                    fn(t, t, **kw)
            with pytest.raises(ValueError, match="^ssim: .*GPU"):      # the default window: the device check, under ssim's name
                fn(t, t)
    loss = torch_ops.SSIMLoss(255.0, "none", 7, 2.0, "uniform")
    assert (loss.data_range, loss.reduction, loss.win_size, loss.win_sigma, loss.window) == (255.0, "none", 7, 2.0, "uniform")
    with pytest.raises(ValueError, match="^ssim: .*GPU"):
        loss(x, x)


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd.torch_ops; "
                        "ssim_amd.torch_ops.SSIMLoss(win_size=7, window='uniform'); ssim_amd.torch_ops.ssim_amp; ssim_amd.torch_ops.ssim_map_amp; "
                        "ssim_amd.make_window(5, 0.8); assert 'torch' not in sys.modules" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the kernels' budgets ----------------------------------------------------------------------------------------------------------------

STRIP_KERNELS, GRAD_KERNELS = 32, 24        # 2 encodings x (R = 1 .. 4 x MAP 0 / 1 x narrow / wide); 2 x (R = 1 .. 4 x A / B / both)


def test_window_16_bit_kernels_never_spill_and_keep_the_budgets_of_the_float32_kernels():
    """Build-time guard, compiled as tests/test_ssimk_cpu.py compiles ssimk_kernels.hip, with that test's budgets: the strip kernels keep
    three waves per SIMD (at most 168 VGPRs, LDS for 12 waves per CU), the gradient kernels two workgroups of 256 lanes per CU (at most 128
    VGPRs, at most 64 KiB of LDS per workgroup), nothing spills, and the file holds 32 + 24 + 1 = 57 kernels, every (encoding, radius)
    with its four strip and three gradient kernels."""
    src = os.path.join(CSRC, "ssimhk_kernels.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
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
    strip = {k: v for k, v in kernels.items() if "ssimhk_strip" in k}
    grad = {k: v for k, v in kernels.items() if "ssimhk_grad" in k}
    reduce_ = [k for k in kernels if "ssimhk_reduce" in k]
    assert len(strip) == STRIP_KERNELS and len(grad) == GRAD_KERNELS and len(reduce_) == 1 and len(kernels) == 57, sorted(kernels)
    for enc in (0, 1):                                             # kSHTypeF16, kSHTypeBF16
        for radius in (1, 2, 3, 4):
            assert len([k for k in strip if "ssimhk_strip_kernelILi%dELi%dE" % (enc, radius) in k]) == 4, (enc, radius, sorted(strip))
            assert len([k for k in grad if "ssimhk_grad_kernelILi%dELi%dE" % (enc, radius) in k]) == 3, (enc, radius, sorted(grad))
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in strip.items():
        assert v["VGPRs"] <= 168 and v["Occupancy"] >= 3 and v["LDS"] <= 13312, (k, v)
    for k, v in grad.items():
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 2 and v["LDS"] <= 65536, (k, v)


# ---- the input condition of the GPU module's rounding test ---------------------------------------------------------------------------

@pytest.mark.parametrize("window", K.WINDOWS, ids=K.name_of)
def test_the_rounding_test_of_the_gpu_module_cannot_pass_vacuously(window):
    """tests/test_gpu_ssimhk.py compares the float16 gradients of ssimhk_inputs.rounding_pair at gOut = G_SMALL and G_LARGE with the
    float32 gradients rounded once.  Here the float64 model's gradient of the same widened planes, rounded to float16: G_SMALL leaves
    subnormals, G_LARGE both Inf and normal numbers -- by the hundred, where the model and the fp32 kernels differ in the last digits."""
    a, b = IN.widened([IN.rounding_pair(HM.F16)], HM.F16)[0]
    small = [IN.census(HM.round_to(np.float32(g), HM.F16), HM.F16) for g in K.grad(a, b, 1.0, IN.G_SMALL, window)]
    large = [IN.census(HM.round_to(np.float32(g), HM.F16), HM.F16) for g in K.grad(a, b, 1.0, IN.G_LARGE, window)]
    print(K.name_of(window), "(subnormal, Inf, normal) of dA, dB: G_SMALL", small, "G_LARGE", large)
    for sub, inf, normal in small:
        assert sub >= 100 and inf == 0
    for sub, inf, normal in large:
        assert inf >= 100 and normal >= 100
