"""CPU: SSIM of float16 / bfloat16 volumes under a caller-chosen window, its gradient and the gradient of its map -- the boundaries of
the rmgr_ssim_hip_*_ssim3h_win* entries (include/rmgr/ssim-hip.h).  Sizes are W x H x D; arrays are (D, H, W); 16-bit samples travel as
uint16 bit patterns.

  * the five entry points are exported, declared and listed; the Python keywords exist;
  * every EINVAL of a window comes before the device, and so does every EINVAL of the entry without _win, under a valid window and NULL;
  * _host without a device is ENODEV;
  * ssim_amd.torch_ops: the window errors of the 3-D _amp names and SSIM3DLoss are those tests/test_ssim3k_cpu.py lists, at every
    dtype; two 16-bit CPU tensors with a window are the "GPU only" TypeError, not "fixed window"; the 2-D names keep "fixed window" and
    ssim3d / ssim3d_map keep "float32 for now"; the import stays torch-free;
  * ssim3hk_kernels.hip never spills, holds seven kernels per (encoding, radius) -- 56 -- and keeps the budgets tests/test_ssim3k_cpu.py
    asserts for the float32 kernels of the same radius (plan3k assumes them);
  * the planner the 16-bit windowed entries launch with is plan3k, seen through ssim3hk_kernels.h: tests/ssim3k_plan.py restates it, and
    nothing about it depends on the size of a sample.
"""
import ctypes
import errno
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ssim3k_plan as PK
import ssim_amd
from conftest import ROOT
from test_ssim3k_cpu import BAD_WINDOWS, GOOD_WINDOWS

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_ssim3h_win", "rmgr_ssim_hip_compute_ssim3h_win_device", "rmgr_ssim_hip_compute_ssim3h_win_host",
                "rmgr_ssim_hip_enqueue_ssim3h_win_grad", "rmgr_ssim_hip_enqueue_ssim3h_win_map_grad")
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


def test_python_keywords_exist_and_take_a_window_only():
    for fn in (ssim_amd.compute_ssim3h, ssim_amd.compute_ssim3h_batch, ssim_amd.Context.ssim3h_device, ssim_amd.Context.enqueue_ssim3h,
               ssim_amd.Context.enqueue_ssim3h_grad, ssim_amd.Context.enqueue_ssim3h_map_grad):
        p = inspect.signature(fn).parameters
        assert "window" in p and p["window"].default is None and list(p)[-1] == "window", fn
    a = np.zeros((2, 3, 4), np.float16)
    with pytest.raises(TypeError):
        ssim_amd.compute_ssim3h(a, a, 1.0, window=(7, 1.5))
    with pytest.raises(TypeError):
        ssim_amd.compute_ssim3h_batch([(a, a)], 1.0, window="uniform")


# ---- the C ABI's validation (no device needed) -----------------------------------------------------------------------------------------

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


def _gmaps(k, n=1):
    gs = (ssim_amd.GradOut3F * n)()
    for i in range(n):
        gs[i] = ssim_amd.GradOut3F(k.ctypes.data, 1, k.shape[2], k.shape[2] * k.shape[1])
    return gs


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    """The fake context and the fake device pointers are never dereferenced: an EINVAL that came after the first use of the context
    would crash.  A valid window with a NULL context is EINVAL too (the entries that need one), which shows the window passed."""
    shape = (6, 20, 30)
    a, b, ga = np.zeros(shape, np.uint16), np.zeros(shape, np.uint16), np.zeros(shape, np.uint16)
    k, m32 = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
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
    # the window: a bad size, a bad kind, sigma 0 / negative / NaN / Inf for a Gaussian
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
    for w in ((7, 1, 0.0), None):
        assert rc(count=0, w=w) == E
        assert (f(fake_ctx, 1, None, F16, 1.0, win(w), out, _grads(ga), None) if grad else f(fake_ctx, 1, None, F16, 1.0, win(w), out)) == E
        assert rc(o=None, w=w) == E
        for dim in ("width", "height", "depth"):
            assert rc(params=_params(a, b, **{dim: 0}), w=w) == E
            assert rc(params=_params(a, b, **{dim: 0x7FFF0001}), w=w) == E
            two = _params(a, b, 2)
            setattr(two[1], dim, getattr(two[1], dim) - 1)
            assert rc(count=2, params=two, w=w) == E
        assert rc(params=_params(a, b, width=0x7FFF0000, height=0x7FFF0000), w=w) == E      # more than 2^24 - 1 tiles
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
        for off in (1, 2, 3):                                      # the map stays 4-byte aligned
            assert rc(params=_params(a, b, ssimMap=m32.ctypes.data + off), w=w) == E
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
    a = np.full((4, 8, 8), 0.25, np.float16)
    if ssim_amd.device_count() > 0:
        v, _ = ssim_amd.compute_ssim3h(a, a, 1.0, window=win)
        assert abs(float(v) - 1.0) < 1e-6
        return
    u = np.zeros((6, 20, 30), np.uint16)
    out = (ctypes.c_float * 1)()
    for st in (F16, BF16):
        assert lib.rmgr_ssim_hip_compute_ssim3h_win_host(None, 1, _params(u, u), st, 1.0, ctypes.byref(win), out) == errno.ENODEV
        assert lib.rmgr_ssim_hip_compute_ssim3h_win_host(None, 1, _params(u, u), st, 1.0, None, out) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError) as e:
        ssim_amd.compute_ssim3h(a, a, 1.0, window=win)
    assert e.value.errno == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError) as e:
        ssim_amd.compute_ssim3h_batch([(u, u), (u, u)], 1.0, sample_type="bfloat16", window=win)
    assert e.value.errno == errno.ENODEV


# ---- torch_ops (CPU tensors) -----------------------------------------------------------------------------------------------------------

def _amp_names(torch_ops):
    return (("ssim3d_amp", torch_ops.ssim3d_amp), ("ssim3d_map_amp", torch_ops.ssim3d_map_amp),
            ("ssim3d_amp", lambda x, y, **kw: torch_ops.SSIM3DLoss(**kw)(x, y)))


def test_torch_ops_window_errors_come_first_at_every_dtype():
    """The lists of tests/test_ssim3k_cpu.py, with float32, float16 and bfloat16 CPU tensors: a bad window is refused before the tensors
    are looked at; a valid one reaches the device check -- ValueError for float32, the "GPU only" TypeError for 16-bit tensors."""
    import torch
    from ssim_amd import torch_ops
    x32 = torch.zeros(2, 1, 8, 16, 16)
    for x in (x32, x32.half(), x32.bfloat16()):
        for name, fn in _amp_names(torch_ops):
            for kw in (dict(win_size=7.0), dict(win_size="7"), dict(win_size=True), dict(window=1), dict(window=None)):
                with pytest.raises(TypeError) as e:
                    fn(x, x, **kw)
                assert "GPU only" not in str(e.value), kw
            for kw in (dict(win_size=4), dict(win_size=13), dict(win_size=1), dict(win_size=-3), dict(win_sigma=0.0), dict(win_sigma=-1.0),
                       dict(win_sigma=float("nan")), dict(win_sigma=float("inf")), dict(window="box"), dict(window="Gaussian")):
                with pytest.raises(ValueError):
                    fn(x, x, **kw)
            for kw in (dict(win_size=7), dict(win_size=3, window="uniform"), dict(window="uniform", win_sigma=float("nan")), dict(win_size=5, win_sigma=0.8), dict()):
                if x.dtype == torch.float32:
                    with pytest.raises(ValueError, match="GPU"):
                        fn(x, x, **kw)
                else:
                    with pytest.raises(TypeError, match="^%s: .*GPU only" % name) as e:
                        fn(x, x, **kw)
                    assert "fixed window" not in str(e.value)


def test_the_other_refusals_stay_as_they_are():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 1, 8, 16, 16)
    for t in (x.half(), x.bfloat16()):
        # the 2-D names keep the fixed window with 16-bit tensors
        for fn in (torch_ops.ssim, torch_ops.ssim_map, lambda a, b, **kw: torch_ops.SSIMLoss(**kw)(a, b)):
            with pytest.raises(TypeError, match="fixed window"):
                fn(t, t, win_size=7)
            with pytest.raises(TypeError, match="fixed window"):
                fn(t, t, window="uniform")
        # the float32-only 3-D names refuse the tensors, with and without a window
        for kw in (dict(win_size=7), dict(win_size=3, window="uniform"), dict()):
            with pytest.raises(TypeError, match="^ssim3d: .*float32 for now"):
                torch_ops.ssim3d(t, t, **kw)
            with pytest.raises(TypeError, match="^ssim3d_map: .*float32 for now"):
                torch_ops.ssim3d_map(t, t, **kw)
        # mixed pairs
        for name, fn in _amp_names(torch_ops):
            for pair in ((x, t), (t, x), (x.half(), x.bfloat16())):
                with pytest.raises(TypeError, match="^%s: two float32, two float16 or two bfloat16" % name):
                    fn(*pair, win_size=7)
    loss = torch_ops.SSIM3DLoss(255.0, "none", 7, 2.0, "uniform")
    assert (loss.data_range, loss.reduction, loss.win_size, loss.win_sigma, loss.window) == (255.0, "none", 7, 2.0, "uniform")


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd.torch_ops; "
                        "ssim_amd.torch_ops.SSIM3DLoss(win_size=7, window='uniform'); ssim_amd.make_window(5, 0.8); "
                        "assert 'torch' not in sys.modules" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the kernels' budgets ----------------------------------------------------------------------------------------------------------------

def test_window_16_bit_volume_kernels_never_spill_and_keep_the_budgets_of_the_float32_kernels():
    """Build-time guard, compiled as tests/test_ssim3k_cpu.py compiles ssim3k_kernels.hip: no scratch; exactly 7 kernels per (encoding,
    radius) -- 4 walks (value, dA, dB, both), 3 adjoint walks --, 56 in all; for every radius the walks use at most 112 VGPRs at 4 waves
    per SIMD or more, the adjoint walks at most 168 VGPRs at 3 waves per SIMD or more, and LDS is at most 16 (16 + 2R)^2 + 256 (16 + 2R)
    + 32 bytes: the budgets of the float32 kernels of the same radius, which plan3k's cost model assumes."""
    src = os.path.join(CSRC, "ssim3hk_kernels.hip")
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
    assert len(kernels) == 56, sorted(kernels)
    for enc in (0, 1):                                             # kSHTypeF16, kSHTypeBF16
        for radius in (1, 2, 3, 4):
            walk = {k: v for k, v in kernels.items() if "ssim3hk_walk_kernelILi%dELi%dE" % (enc, radius) in k}
            adjoint = {k: v for k, v in kernels.items() if "ssim3hk_adjoint_kernelILi%dELi%dE" % (enc, radius) in k}
            assert len(walk) == 4 and len(adjoint) == 3, (enc, radius, sorted(kernels))
            lds = 16 * (16 + 2 * radius) ** 2 + 256 * (16 + 2 * radius) + 32
            for k, v in walk.items():
                assert v["ScratchSize"] == 0 and v["VGPRs"] <= 112 and v["Occupancy"] >= 4 and v["LDS"] <= lds, (k, v)
            for k, v in adjoint.items():
                assert v["ScratchSize"] == 0 and v["VGPRs"] <= 168 and v["Occupancy"] >= 3 and v["LDS"] <= lds, (k, v)


# ---- the planner ----------------------------------------------------------------------------------------------------------------------

def test_the_planner_of_the_16_bit_entries_is_plan3k_and_knows_no_sample_size(tmp_path):
    """tests/src/plan3k_probe.cpp built with ssim3hk_kernels.h in front of it: the plan3k the 16-bit windowed entries see through that
    header is the one tests/ssim3k_plan.py restates (tests/test_ssim3k_cpu.py holds it to the float32 entries' header), for every
    radius, 17 x 17 x 131 at the counts the GPU module launches included.  Its arguments are radius, W, H, D, count and CUs -- no sample
    size --, and the volume host flow (ssim_volumes_abi.cpp: one forward and one gradient, serving both sample types) plans every launch
    with exactly those."""
    obj3f = "build/obj/ssim3f_kernels.o"
    r = subprocess.run(["make", "-C", ROOT, obj3f], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    obj, exe = str(tmp_path / "plan3hk_probe.o"), str(tmp_path / "plan3hk_probe")
    src = os.path.join(ROOT, "tests", "src", "plan3k_probe.cpp")
    for cmd in ([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                 "-include", os.path.join(CSRC, "ssim3hk_kernels.h"), "-c", src, "-o", obj],
                [HIPCC, "--offload-arch=gfx950", obj, os.path.join(ROOT, obj3f), "-o", exe]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(2025)
    rows = []
    for radius in (1, 2, 3, 4, 5):
        for _ in range(40):
            w, h, d = int(rng.integers(1, 300)), int(rng.integers(1, 300)), int(rng.integers(1, 1300))
            rows.append((radius, w, h, d, int(np.exp(rng.uniform(0, np.log(70000.0)))), int(rng.choice([32, 64, 256, 304, 0]))))
        rows += [(radius, 17, 17, 131, n, cus) for n in (1, 5, 16, 31, 61, 154) for cus in (256, 304)]
    text = "".join("%d %d %d %d %d %d\n" % row for row in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(rows)
    for row, g in zip(rows, got):
        assert PK.Geometry(*g[:5]) == PK.plan3k(*row), (row, g)
        assert g[5] == PK.max_count(*row[1:4]), row
    # no sample size anywhere: the restatement's and the C++ planner's arguments, and the calls of the 16-bit host flow
    assert list(inspect.signature(PK.plan3k).parameters) == ["radius", "width", "height", "depth", "count", "cus"]
    with open(os.path.join(CSRC, "ssim3k_kernels.h")) as f:
        assert re.search(r"plan3k\(uint32_t radius, uint32_t width, uint32_t height, uint32_t depth, uint32_t count, int cu_count\)", f.read())
    with open(os.path.join(CSRC, "ssim_volumes_abi.cpp")) as f:
        abi = f.read()
    calls = re.findall(r"plan3k\(([^)]*)\)", abi)
    assert len(calls) == 2 and all(c == "win.radius, W, H, D, n, c->cu_count" for c in calls), calls
    assert re.findall(r"plan3f\(([^)]*)\)", abi) == ["W, H, D, 1, 0"]             # the cells of one volume, for the partials: no launch
