"""CPU: SSIM of float32 samples under a caller-chosen window -- the definition and its boundaries (include/rmgr/ssim-hip.h,
rmgr_ssim_hip_Window and rmgr_ssim_hip_*_ssimf_win*).

  * the taps rule: {11, 1.5} is the engine's window bit for bit, box taps, every window sums to 1 within a few float ulps;
  * the float64 model (tests/ssimk_model.py) is ssimf_model / ssimw_model at the default window, exactly, and agrees with an independent
    float64 restatement for the others: torch on the CPU, F.conv2d on replicate-padded input plus autograd;
  * the fp32 emulation of the kernels stays inside the bounds tests/test_gpu_ssimk.py asserts, per window;
  * the entry points are exported, every new EINVAL comes before the device, a valid call without a device is ENODEV, and
    ssim_amd.torch_ops refuses what it documents before any GPU call;
  * the new kernels never spill and keep their occupancy.
"""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import ssimf_model as M
import ssimk_model as K
import ssimw_model as MW
import ssim_amd
from conftest import ROOT, load_pair

ENTRY_POINTS = ("rmgr_ssim_hip_enqueue_ssimf_win", "rmgr_ssim_hip_compute_ssimf_win_device", "rmgr_ssim_hip_compute_ssimf_win_host",
                "rmgr_ssim_hip_enqueue_ssimf_win_grad", "rmgr_ssim_hip_enqueue_ssimf_win_map_grad")


def unit_pair(manifest, name="bbb257x65_q50_ch1"):
    a, b = load_pair(manifest[name])
    return a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)


# ---- the taps ----

def test_taps_rule():
    assert np.array_equal(K.full_taps(K.DEFAULT), M.gaussian_taps())            # the engine's taps, bit for bit
    assert np.array_equal(K.taps(K.DEFAULT), M.gaussian_taps().astype(np.float32)[5:])
    for size in K.SIZES:
        box = K.taps((size, 123.0, "uniform"))                                   # sigma is ignored
        assert box.dtype == np.float32 and len(box) == (size + 1) // 2 and np.all(box == np.float32(1.0 / size))
    for window in K.WINDOWS + (K.DEFAULT, (3, 0.5, "gaussian"), (9, 40.0, "gaussian"), (5, 0.05, "gaussian")):
        g = K.full_taps(window)
        assert len(g) == window[0] and np.array_equal(g, g[::-1]) and np.all(g >= 0) and g[len(g) // 2] == g.max()
        assert abs(float(g.sum()) - 1.0) <= 4 * 2.0 ** -24, (window, float(g.sum()))         # a few float ulps of 1
    # sigma enters as the float the C ABI receives
    assert np.array_equal(K.taps((7, 0.1, "gaussian")), K.taps((7, float(np.float32(0.1)), "gaussian")))


# ---- the model ----

def test_model_at_the_default_window_is_ssimf_model_and_ssimw_model_exactly(manifest):
    a, b = unit_pair(manifest)
    v, m = K.ssim(a, b, 1.0)
    v0, m0 = M.ssim(a, b, 1.0)
    assert v == v0 and np.array_equal(m, m0)
    for got, want in zip(K.grad(a, b, 1.0, -0.75), M.grad(a, b, 1.0, -0.75)):
        assert np.array_equal(got, want)
    plane = next(K.upstream_planes(*a.shape))[1]
    for got, want in zip(K.grad_map(a, b, 1.0, plane), MW.grad_map(a, b, 1.0, plane)):
        assert np.array_equal(got, want)
    e, e0 = K.emulate_fp32(a, b, 1.0, g_out=-0.75), M.emulate_fp32(a, b, 1.0, -0.75)
    assert e[0] == e0[0] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(e[1:], e0[1:]))
    for got, want in zip(K.emulate_fp32(a, b, 1.0, gmap=plane)[2:], MW.emulate_fp32_map_grad(a, b, 1.0, plane)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(K.adjoint_weights(7, K.taps()), M.adjoint_weights(7, K.taps()))


def test_gt_is_the_adjoint_of_g_for_every_window():
    rng = np.random.default_rng(12)
    for window in K.WINDOWS:
        for shape in [(20, 24), (30, 3), (3, 7), (5, 1), (1, 1), (2, 1), (6, 6)]:
            u, v = rng.standard_normal(shape), rng.standard_normal(shape)
            lhs, rhs = float(np.sum(K.blur(u, window) * v)), float(np.sum(u * K.blur_t(v, window)))
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-3), (window, shape, lhs, rhs)


def test_adjoint_weights_sum_like_the_clamped_window():
    for window in K.WINDOWS:
        g = K.taps(window)
        R = len(g) - 1
        for n in (1, 2, R, R + 1, 2 * R, 2 * R + 1, 2 * R + 2, 40):
            w = K.adjoint_weights(n, g).astype(np.float64)
            dense = np.zeros((n, n))
            for j in range(-R, R + 1):
                for q in range(n):
                    if 0 <= q + j < n:
                        dense[q, q + j] += w[j + R, q]
            want = np.zeros((n, n))
            for p in range(n):
                for t in range(-R, R + 1):
                    want[min(max(p + t, 0), n - 1), p] += float(g[abs(t)])
            assert np.abs(dense - want).max() < 1e-7, (window, n)


CONV_WINDOWS = ((3, 0.0, "uniform"), (7, 0.0, "uniform"), (7, 1.5, "gaussian"), (11, 2.0, "gaussian"), (5, 0.8, "gaussian"))


def conv2d_restatement(torch, a, b, data_range, window, upstream):
    """An independent float64 statement of the definition: F.conv2d with the outer product of the taps on replicate-padded input, the
    formula, and autograd for the derivative of sum(upstream * map) (upstream a plane) or of upstream * mean(map) (a scalar)."""
    import torch.nn.functional as Fn
    g = torch.tensor(K.full_taps(window), dtype=torch.float64)
    R = K.radius(window)
    k2 = (g[:, None] * g[None, :])[None, None]
    x = torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    y = torch.tensor(np.asarray(b, np.float64), requires_grad=True)

    def blur(t):
        return Fn.conv2d(Fn.pad(t[None, None], (R, R, R, R), mode="replicate"), k2)[0, 0]
    c1, c2 = K.constants(data_range)
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    m = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    loss = (torch.tensor(np.asarray(upstream, np.float64)) * m).sum() if np.ndim(upstream) == 2 else float(upstream) * m.mean()
    loss.backward()
    return float(m.detach().mean()), m.detach().numpy(), x.grad.numpy(), y.grad.numpy()


@pytest.mark.parametrize("window", CONV_WINDOWS, ids=K.name_of)
def test_model_agrees_with_the_conv2d_restatement(manifest, window):
    """Both sides are float64 and differ only in summation order: 1e-9 of the largest magnitude."""
    import torch
    a, b = unit_pair(manifest, "bbb255x63_q50_ch1")
    crops = [(a[:40, :48], b[:40, :48], 1.0), (a[5:8, 100:105] * 255, b[5:8, 100:105] * 255, 255.0), (a[:1, :1], b[:1, :1], 1.0),
             (a[10:12, 7:8], b[10:12, 7:8], 1.0)]
    for ca, cb, r in crops:
        h, w = ca.shape
        plane = np.random.default_rng(h * 100 + w).standard_normal((h, w))
        v, m, ga, gb = conv2d_restatement(torch, ca, cb, r, window, -0.75)
        _, _, pa, pb = conv2d_restatement(torch, ca, cb, r, window, plane)
        mv, mm = K.ssim(ca, cb, r, window)
        assert abs(mv - v) <= 1e-9 and np.abs(mm - m).max() <= 1e-9 * np.abs(m).max(), (window, ca.shape)
        for got, want in zip(K.grad(ca, cb, r, -0.75, window) + K.grad_map(ca, cb, r, plane, window), (ga, gb, pa, pb)):
            assert np.abs(got - want).max() <= 1e-9 * max(np.abs(want).max(), 1e-300), (window, ca.shape)


# ---- the emulation against the model ----

@pytest.mark.parametrize("window", K.WINDOWS, ids=K.name_of)
def test_fp32_emulation_is_inside_the_gpu_bounds(manifest, window):
    """emulate_fp32 against the float64 model over ssimk_model.FIXTURES in the forms "unit" and "raw": every pixel, the value, the map and
    both gradients for the scalar upstream gradient and for a standard-normal and a one-hot plane, and the pair of identical images.
    ssimk_model.EMU holds the figures per window; tests/test_gpu_ssimk.py asserts twice these."""
    got = K.measure(manifest, window)
    print("%s: px %.3g global %.3g grad %.3g identical %.3g" % ((K.name_of(window),) + got))
    for v, emu, tol in zip(got, K.EMU[window], K.tolerances(window)):
        assert v <= emu, (window, got, K.EMU[window])
        # pinned from below as well: a figure that moved far away means the emulation no longer restates these kernels
        assert v >= emu / 2, (window, got, K.EMU[window])
        assert 1.9 <= tol / emu <= 2.2


def test_default_window_reproduces_the_ssimf_figures(manifest):
    """The default window's emulation IS ssimf_model's (bit for bit, above): its figures are ssimf_model.EMU_*."""
    a, b = load_pair(manifest["bbb255x63_q50_ch1"])
    for _, fa, fb, r in M.forms(a, b):
        e, e0 = K.emulate_fp32(fa, fb, r, K.DEFAULT, g_out=1.0), M.emulate_fp32(fa, fb, r, 1.0)
        assert e[0] == e0[0] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(e[1:], e0[1:]))


# ---- the C ABI's validation (no device needed) ----

def _params(a, b, n=1, **over):
    ps = (ssim_amd.ParamsF * n)()
    h, w = a.shape
    for i in range(n):
        ps[i] = ssim_amd.make_params_f(w, h, a.ctypes.data, 1, w, b.ctypes.data, 1, w)
    for k, v in over.items():
        setattr(ps[0], k, v)
    return ps


def _grads(a, n=1):
    gs = (ssim_amd.GradF * n)()
    for i in range(n):
        gs[i] = ssim_amd.GradF(a.ctypes.data, 1, a.shape[1])
    return gs


def test_entry_points_are_exported(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in ssim_amd.C_SYMBOLS
    for name in ("Window", "make_window", "WINDOW_GAUSSIAN", "WINDOW_UNIFORM"):
        assert hasattr(ssim_amd, name)
    assert lib.rmgr_ssim_hip_get_abi_version() == 6
    assert ctypes.sizeof(ssim_amd.Window) == 12
    w = ssim_amd.make_window(7, 1.5)
    assert (w.size, w.kind, w.sigma) == (7, ssim_amd.WINDOW_GAUSSIAN, 1.5)
    w = ssim_amd.make_window(3, kind="uniform")
    assert (w.size, w.kind) == (3, ssim_amd.WINDOW_UNIFORM)
    for bad, exc in (((4,), ValueError), ((13,), ValueError), ((1,), ValueError), ((7, 0.0), ValueError), ((7, float("nan")), ValueError),
                     ((7, float("inf")), ValueError), ((7, -1.0), ValueError), ((7, 1.5, "box"), ValueError), ((7.0,), TypeError),
                     ((True,), TypeError), ((7, 1.5, 1), TypeError)):
        with pytest.raises(exc):
            ssim_amd.make_window(*bad)


def _call(lib, fn, ctx, count, ps, r, win, out, grads=None, maps=None):
    f = getattr(lib, fn)
    wp = None if win is None else ctypes.byref(win)
    if fn.endswith("_map_grad"):
        return f(ctx, count, ps, r, wp, maps, grads[0], grads[1])
    if fn.endswith("_grad"):
        return f(ctx, count, ps, r, wp, out, grads[0], grads[1])
    return f(ctx, count, ps, r, wp, out)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_einval_comes_before_the_device(lib, fn):
    a = np.zeros((20, 30), np.float32)
    ga = np.zeros((20, 30), np.float32)
    out = (ctypes.c_float * 4)() if not fn.startswith("rmgr_ssim_hip_enqueue") else ctypes.c_void_p(16)   # never dereferenced
    fake_ctx = None if fn.endswith("_host") else ctypes.c_void_p(1)                                     # never dereferenced
    maps = (ssim_amd.GradOutF * 1)()
    maps[0] = ssim_amd.GradOutF(ga.ctypes.data, 1, 30)
    E = errno.EINVAL

    def rc(win, count=1, ps=None, r=1.0, o=out, ctx=fake_ctx, grads=None, m=maps):
        return _call(lib, fn, ctx, count, _params(a, a) if ps is None else ps, r, win, o, (_grads(ga), None) if grads is None else grads, m)
    W = ssim_amd.Window
    # the new ones: a size outside the five, an unknown kind, a Gaussian sigma that is not finite or not > 0
    for size in (0, 1, 2, 4, 6, 8, 10, 12, 13, 0xFFFFFFFF):
        assert rc(W(size, 0, 1.5)) == E and rc(W(size, 1, 1.5)) == E, size
    for kind in (2, 3, 0xFFFFFFFF):
        assert rc(W(7, kind, 1.5)) == E, kind
    for sigma in (0.0, -0.0, -1.5, float("inf"), float("-inf"), float("nan")):
        for size in K.SIZES:
            assert rc(W(size, 0, sigma)) == E, (size, sigma)
    # the ones of the entry without _win still hold under a valid window and under NULL
    for win in (W(7, 0, 1.5), W(3, 1, float("nan")), W(11, 0, 2.0), None):
        assert rc(win, count=0) == E
        assert rc(win, r=0.0) == E and rc(win, r=float("nan")) == E
        assert rc(win, ps=_params(a, a, width=0)) == E
        bad = _params(a, a)
        bad[0].imgA.topLeft = a.ctypes.data + 2
        assert rc(win, ps=bad) == E
        if fn.endswith("_map_grad"):
            assert rc(win, m=None) == E
        else:
            assert rc(win, o=None) == E
        if not fn.endswith("_host"):
            assert rc(win, ctx=None) == E                                          # these entries need a context
        if fn.endswith("_grad"):
            assert rc(win, grads=(None, None)) == E


def test_valid_call_without_a_device_fails_loudly(lib):
    a = np.full((8, 8), 0.25, np.float32)
    if ssim_amd.device_count() > 0:
        v, _ = ssim_amd.compute_ssimf(a, a, 1.0, window=ssim_amd.make_window(3, kind="uniform"))
        assert abs(float(v) - 1.0) < 1e-6
        return
    out = (ctypes.c_float * 1)()
    for win in (ssim_amd.Window(3, 1, 0.0), ssim_amd.Window(7, 0, 1.5), ssim_amd.Window(11, 0, 2.0), ssim_amd.Window(11, 1, float("nan")), None):
        wp = None if win is None else ctypes.byref(win)
        assert lib.rmgr_ssim_hip_compute_ssimf_win_host(None, 1, _params(a, a), 1.0, wp, out) == errno.ENODEV
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssimf(a, a, 1.0, window=ssim_amd.make_window(7, 1.5))
    with pytest.raises(ssim_amd.SsimError):
        ssim_amd.compute_ssimf_batch([(a, a), (a, a)], 1.0, window=ssim_amd.make_window(3, kind="uniform"))
    with pytest.raises(TypeError):
        ssim_amd.compute_ssimf(a, a, 1.0, window=(7, 1.5))


def test_torch_ops_refuses_what_it_documents_before_any_gpu_call():
    import torch
    from ssim_amd import torch_ops
    x = torch.zeros(2, 3, 16, 16)
    for fn in (torch_ops.ssim, torch_ops.ssim_map, lambda x, y, **kw: torch_ops.SSIMLoss(**kw)(x, y)):
        for kw in (dict(win_size=7.0), dict(win_size="7"), dict(win_size=True), dict(window=1), dict(window=None)):
            with pytest.raises(TypeError):
                fn(x, x, **kw)
        for kw in (dict(win_size=4), dict(win_size=13), dict(win_size=1), dict(win_size=-3), dict(win_sigma=0.0), dict(win_sigma=-1.0),
                   dict(win_sigma=float("nan")), dict(win_sigma=float("inf")), dict(window="box"), dict(window="Gaussian")):
            with pytest.raises(ValueError):
                fn(x, x, **kw)
        for t in (x.half(), x.bfloat16()):
            for kw in (dict(win_size=7), dict(win_sigma=2.0), dict(window="uniform"), dict(win_size=3, window="uniform")):
                with pytest.raises(TypeError, match="fixed window"):
                    fn(t, t, **kw)
        # valid windows reach the device check: CPU tensors
        for kw in (dict(win_size=7), dict(win_size=3, window="uniform"), dict(window="uniform", win_sigma=float("nan")), dict()):
            with pytest.raises(ValueError, match="GPU"):
                fn(x, x, **kw)
    with pytest.raises(ValueError):
        torch_ops.SSIMLoss(win_size=6)                                         # checked at construction
    with pytest.raises(TypeError):
        torch_ops.SSIMLoss(window=7)


def test_import_stays_torch_free():
    r = subprocess.run(["python3", "-c", "import sys; sys.path.insert(0, %r); import ssim_amd, ssim_amd.torch_ops; "
                        "ssim_amd.make_window(7, 1.5); assert 'torch' not in sys.modules" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


STRIP_KERNELS, GRAD_KERNELS = 16, 12        # R = 1 .. 4 x MAP 0 / 1 x narrow / wide; R = 1 .. 4 x A / B / both


def test_window_kernels_never_spill_and_keep_their_occupancy():
    """Build-time guard, as tests/test_ssimf_cpu.py has for ssimf_kernels.hip, with that file's budgets: the strip kernels keep three
    waves per SIMD (at most 168 VGPRs, LDS for 12 waves per CU), the gradient kernels two workgroups of 256 lanes per CU (at most 128
    VGPRs, at most 64 KiB of LDS per workgroup), nothing spills, and the file holds the 29 kernels DESIGN.md section 16 lists."""
    src = os.path.join(ROOT, "ssim_amd", "csrc", "ssimk_kernels.hip")
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
    strip = {k: v for k, v in kernels.items() if "ssimk_strip" in k}
    grad = {k: v for k, v in kernels.items() if "ssimk_grad" in k}
    assert len(strip) == STRIP_KERNELS and len(grad) == GRAD_KERNELS and len(kernels) == STRIP_KERNELS + GRAD_KERNELS + 1, sorted(kernels)   # + the reduction
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in strip.items():
        assert v["VGPRs"] <= 168 and v["Occupancy"] >= 3 and v["LDS"] <= 13312, (k, v)
    for k, v in grad.items():
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 2 and v["LDS"] <= 65536, (k, v)
